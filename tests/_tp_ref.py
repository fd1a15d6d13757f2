"""The stage kit (tests/_model_ref.py) extended to the tensor-parallel forms of picotron_amd/functional.py: a recorder of
the collectives beside the kernel calls, an issue / wait ledger, the cross-rank roles, and the stages of the
sequence-parallel and replicated layers, the vocab-parallel entry, exit and cross-entropy.

Recorder (`recording_collectives`)
    The functional.TPContext methods all_reduce, all_gather_rows_into, reduce_scatter_rows and
    reduce_scatter_rows_into (gather_chunk, scatter_chunk and all_gather_rows go through the two _into methods)
    log into the SAME ordered list as the K calls of `_model_ref.recording`: a `Call` whose `ins` / `outs` are `Rec`s
    (identity = data_ptr / shape / stride / dtype; an input's `pre` clone taken at the issue, an output's `post`
    clone taken where the collective is complete: at the return of a synchronous call, else in `wait`).  An
    asynchronous call returns a `Handle` whatever the transport returned (gloo's list forms return None): its
    `wait()` forwards to the real handle and logs a `wait` event, so the host order in which production waits is
    on record although gloo has finished long before.  `functional._grad_ready` logs a `grad_ready` event, and
    every DecoderLayer a `node_end` event where its autograd node returns (forward: a module hook; backward: a
    hook on the gradient of the layer's input).

Ledger (`check_waits`)
    From its issue to its `wait` no K call and no other collective may touch a byte range overlapping a
    collective's output, none may write one overlapping its input, and every handle is waited exactly once
    before its node returns.  It works on the Recs' identities alone.  What a K call writes: its results, the
    arguments whose bits differ between their `pre` and `post` clones, and the keyword arguments that name an
    output.  It pins the HOST order; a missing stream dependency under RCCL is out of its sight.

Roles of one rank (`extract_tp`, or the CPU emulation `emu_tp`): {W, rank, c, sp, layers: [{s, ch}], head}
    s      the layer's roles on this rank's token rows (T / W rows in the sequence-parallel form, all T rows
           in the replicated one): x, h1, rstd1, a (the summed attention output), z, h2, rstd2, mr, out, dout, dh2,
           dz, dh1, dx, dw1, dw2
    ch[j]  chunk j's block roles on the gathered rows with this rank's weight shards -- the names of
           _model_ref's stages: h1, qkv_raw, qkv, o, lse, a (this rank's partial), h2, gu, hh, m (partial), dout, dhh,
           dgu, dW_d, dh2 (partial), dW_g, dW_u, dz, do, dqkv_unrot, dqkv_rot, dqkv, dW_o, dh1 (partial), dW_q / k / v
    Every rank's roles are exchanged as CPU tensors (`exchange`); each rank checks its own stages (`check_tp`).

Stages: the shard-local ones are _model_ref's, on the local shapes; what is new here
    layout   a gathered buffer equals, by bits, the concatenation of every rank's shard rows: the flattened
             [T, H] rows are c chunks, rank r holds rows [r n, (r + 1) n) of each, n = T / (c W) (`layout`).
    sums     a reduce-scatter / all-reduce output against the float64 sum of the ranks' recorded partials at
             this rank's rows (`check_sum`): W = 2: bf16(a0 + a1) by bits (one rounding, commutative); W > 2:
             (W - 1) 2^-9 sum |a_i| per element (each of the W - 1 adds rounds a partial sum no larger than
             sum |a_i|); 2^-24 for f32.  Which ranks, which rows, where they land -- not the transport's order.
    norm dW  sequence parallelism: the column sum over every rank's rows from each rank's recorded (dy, z, rstd),
             under _row_ref.dw_target_bound with the ranks' summed bounds plus the f32 sum bound above; the same
             bits on every rank.  The final norm's is local, and no collective may touch it.
    ce       the 16-byte parts (max, sum-exp, target logit, own) against this rank's logits shard: max, target logit
             and own by bits, max + log sum-exp under the statistics' bound (_row_ref.merge_stats + ref_ce_fwd's, the
             composition _model_ref documents for the statistics LSE); row_lse / loss / ce_scale through
             _model_ref's stages on the logits and statistics assembled from every rank's shard; dlogits on this
             rank's columns of their reference.

CPU emulation (`emu_tp`): W ranks in one process, shard weights, the partials summed here in the documented layout,
the same roles as a recorded run; FAULTS injects the wiring mistakes the checker must reject at the named stage, and
`EmuTrace` writes one rank's call and collective log in production's order for the ledger
(tests/test_tp_stage_checker_cpu.py).
"""
import contextlib
import types

import torch

from tests import _gemm_ref as G
from tests import _model_ref as M
from tests import _optim_ref as OR
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
cpu, Call, Rec = M.cpu, M.Call, M.Rec
COLLECTIVES = ("all_reduce", "all_gather_rows_into", "reduce_scatter_rows", "reduce_scatter_rows_into")
EVENTS = ("wait", "node_end", "grad_ready")
FAILS = None   # a list: check_tp(keep_going=True) collects the failing stages here and goes on
OVER = []   # sums over their bound in this process (check_sum), raised together at the end of check_tp
OUT_KW = ("dq", "dk", "dv", "dg", "du", "dx", "dw_out", "out")   # keyword arguments of K calls that name an output


# ============================================================================== recorder of the collectives
class Handle:
    """What an asynchronous collective returned, as production sees it: wait() forwards and logs."""

    def __init__(self, log, call, real, keep):
        self.log, self.call, self.real, self.keep = log, call, real, keep   # keep: the buffers stay allocated

    def wait(self):
        if self.real is not None:
            self.real.wait()
        for r in self.call.outs:
            if r.post is None:
                r.post = r.obj.detach().clone()
        ev = Call("wait", (), {})
        ev.of = self.call
        self.log.append(ev)


def coll_call(name, ins, outs, sync, rank, world):
    c = Call(name, (), {})
    c.coll, c.ins, c.outs, c.sync, c.rank, c.world = True, ins, outs, sync, rank, world
    return c


def is_coll(c):
    return getattr(c, "coll", False)


def _in(t):
    return Rec(t, t.detach().clone())


def _out(t):
    return Rec(t, None)


def _finish(log, call, real, sync, keep):
    log.append(call)
    if sync:
        if real is not None:
            real.wait()
        for r in call.outs:
            r.post = r.obj.detach().clone()
        return None
    call.result = None
    return Handle(log, call, real, keep)


@contextlib.contextmanager
def recording_collectives(rec, model=None, params=None):
    """The collectives of functional.TPContext, functional._grad_ready and (model given) the decoder layers' node
    boundaries logged into rec.calls for the block.  params: {id(parameter): name} for the grad_ready events."""
    from picotron_amd import functional as FN
    TP, log = FN.TPContext, rec.calls
    real = {n: getattr(TP, n) for n in COLLECTIVES}
    real_ready = FN._grad_ready

    def all_reduce(self, t, async_op=False):
        if self.world_size == 1:
            return real["all_reduce"](self, t, async_op)
        call = coll_call("all_reduce", [_in(t)], [_out(t)], not async_op, self.rank, self.world_size)
        h = real["all_reduce"](self, t, async_op)
        return _finish(log, call, h, not async_op, (t,))

    def all_gather_rows_into(self, out, t, async_op=False):
        call = coll_call("all_gather_rows_into", [_in(t)], [_out(out)], not async_op, self.rank, self.world_size)
        h = real["all_gather_rows_into"](self, out, t, async_op)
        return _finish(log, call, h, not async_op, (out, t))

    def reduce_scatter_rows(self, t, async_op=False):
        if self.world_size == 1:
            return real["reduce_scatter_rows"](self, t, async_op)
        ins = [_in(t)]
        out, h = real["reduce_scatter_rows"](self, t, async_op)
        call = coll_call("reduce_scatter_rows", ins, [_out(out)], not async_op, self.rank, self.world_size)
        return out, _finish(log, call, h, not async_op, (out, t))

    def reduce_scatter_rows_into(self, out, t, async_op=False):
        call = coll_call("reduce_scatter_rows_into", [_in(t)], [_out(out)], not async_op, self.rank, self.world_size)
        h = real["reduce_scatter_rows_into"](self, out, t, async_op)
        return _finish(log, call, h, not async_op, (out, t))

    def grad_ready(p):
        ev = Call("grad_ready", (), {})
        ev.param = (params or {}).get(id(p), id(p))
        log.append(ev)
        return real_ready(p)

    def node_end(kind, i):
        ev = Call("node_end", (), {})
        ev.kind, ev.layer = kind, i
        log.append(ev)

    hooks = []
    for i, layer in enumerate(model.decoder_layers if model is not None else ()):
        def pre(mod, args, i=i):
            if args[0].requires_grad:
                args[0].register_hook(lambda g, i=i: node_end("bwd", i))
        hooks.append(layer.register_forward_pre_hook(pre))
        hooks.append(layer.register_forward_hook(lambda mod, args, out, i=i: node_end("fwd", i)))
    for n, f in (("all_reduce", all_reduce), ("all_gather_rows_into", all_gather_rows_into),
                 ("reduce_scatter_rows", reduce_scatter_rows), ("reduce_scatter_rows_into", reduce_scatter_rows_into)):
        setattr(TP, n, f)
    FN._grad_ready = grad_ready
    try:
        yield rec
    finally:
        for n, f in real.items():
            setattr(TP, n, f)
        FN._grad_ready = real_ready
        for h in hooks:
            h.remove()


# ============================================================================== the issue / wait ledger
def extent(rec):
    """The byte range [lo, hi) a Rec's view spans (None: no element)."""
    ptr, shape, stride, dtype = rec.key
    if any(s == 0 for s in shape):
        return None
    span = sum((s - 1) * st for s, st in zip(shape, stride)) + 1
    return ptr, ptr + span * torch.empty((), dtype=dtype).element_size()


def _overlap(a, b):
    return a is not None and b is not None and a[0] < b[1] and b[0] < a[1]


def _changed(r):
    if r.pre is None or r.post is None or r.pre is r.post:
        return False
    return not torch.equal(R.ibits(cpu(r.pre).contiguous()), R.ibits(cpu(r.post).contiguous()))


def touches(call):
    """(the Recs a logged call reads, the Recs it writes)."""
    if is_coll(call):
        return list(call.ins), list(call.outs)
    reads = list(M._flat((call.args, call.kwargs)))
    writes = list(M._flat(call.result)) + [r for r in reads if _changed(r)]
    writes += [r for k in OUT_KW for r in M._flat(call.kwargs.get(k))]
    return reads, writes


def check_waits(calls):
    """The ledger over a recorded (or emulated) trace; returns the number of collectives that were in flight."""
    open_, waited, n = {}, {}, 0
    for i, c in enumerate(calls):
        if c.name == "wait":
            k = id(c.of)
            assert waited.get(k, 0) == 0 and k in open_, \
                f"wait ledger: call {i}: the handle of {c.of.name} (rank {c.of.rank}) is waited a second time"
            waited[k] = 1
            del open_[k]
            continue
        if c.name == "node_end":
            assert not open_, (f"wait ledger: call {i}: the {c.kind} node of layer {c.layer} returns with the handle of "
                               f"{next(iter(open_.values())).name} never waited")
            continue
        if c.name in EVENTS:
            continue
        reads, writes = touches(c) if open_ else ((), ())
        for o in open_.values():
            for r in reads + writes:
                for w in o.outs:
                    assert not _overlap(extent(r), extent(w)), \
                        (f"wait ledger: call {i} ({c.name}) touches {tuple(r.key[1])} at {r.key[0]:#x}, the output of "
                         f"{o.name} issued before it and not yet waited for")
            for r in writes:
                for w in o.ins:
                    assert not _overlap(extent(r), extent(w)), \
                        (f"wait ledger: call {i} ({c.name}) writes {tuple(r.key[1])} at {r.key[0]:#x}, the input of "
                         f"{o.name} issued before it and not yet waited for")
        if is_coll(c) and not c.sync:
            open_[id(c)] = c
            n += 1
    assert not open_, f"wait ledger: the handle of {next(iter(open_.values())).name} is never waited"
    return n


# ============================================================================== layout and sums
def layout(shards, c):
    """Every rank's shard rows [T / W, ...] -> the [T, ...] rows, written out from the documented layout: the T rows
    are c chunks; rank r holds rows [r n, (r + 1) n) of each chunk, n = T / (c W), chunk after chunk."""
    W = len(shards)
    n = shards[0].shape[0] // c
    return torch.cat([shards[r][j * n:(j + 1) * n] for j in range(c) for r in range(W)])


def my_rows(full, W, rank, c):
    """The inverse: this rank's rows of the [T, ...] rows."""
    Tc = full.shape[0] // c
    n = Tc // W
    return torch.cat([full[j * Tc + rank * n:j * Tc + (rank + 1) * n] for j in range(c)])


def check_layout(role, got, shards, c, tag):
    R.check_exact(f"{role} (layout of the gathered rows)", got, layout(shards, c))
    return 0.0


def check_sum(role, got, partials, tag):
    """got: this rank's rows of the sum over the ranks of `partials` (each already cut to those rows)."""
    W = len(partials)
    dt = got.dtype
    assert all(p.dtype == dt and p.shape == got.shape for p in partials), f"{role}: the partials' dtype / shape"
    if W == 2:
        return R.check_exact(role, got, (partials[0].to(F64) + partials[1].to(F64)).to(F32).to(dt))
    s = sum(p.to(F64) for p in partials)
    mass = sum(p.to(F64).abs() for p in partials)
    u = 2.0 ** -9 if dt == BF else 2.0 ** -24
    try:
        return R.check(role, got, s, (W - 1) * u * mass, tag)
    except AssertionError as e:   # reported at the end of check_tp: the stages behind this one are still checked
        if "over the bound" not in str(e):
            raise
        OVER.append(str(e))
        return R.WORST[(tag, role)]


# ============================================================================== the tensor-parallel stages
CHUNK_ATTN_FWD = ("qkv_raw", "qkv", "o", "a")
CHUNK_MLP_FWD = ("gu", "hh")
CHUNK_MLP_BWD = ("dhh", "dgu", "dW_d", "dh2", "dW_g")
CHUNK_ATTN_BWD = ("do", "dW_o", "dqkv_unrot", "dqkv_rot", "dh1", "")


def _stages(names):
    all_ = M.LAYER_FWD + M.LAYER_BWD
    return [s for n in names for s in all_ if (s.produces[0] if s.produces else "") == n]


def _s_m(r, c, tag):
    """The down projection's partial: hh W_d^T, with the residual z in the epilogue iff the role carries one."""
    if r.get("m_res") is not None:
        return M._gemm("m", r["m"], r["hh"], c.wd.t(), tag, G.EPI_BF16_RES, residual=r["m_res"])
    return M._gemm("m", r["m"], r["hh"], c.wd.t(), tag)


def _run(out, prefix, roles, c, stages, form):
    """_model_ref.check_stages stage by stage; a failure names the layer and the chunk."""
    for st in stages:
        try:
            res = M.check_stages(roles, c, [st], form)
        except AssertionError as e:
            msg = str(e)
            msg = f"stage {prefix}{msg[len('stage '):]}" if msg.startswith("stage ") else f"stage {prefix}: {msg}"
            if FAILS is None:
                raise AssertionError(msg) from None
            FAILS.append(msg)
            continue
        for k, v in res.items():
            out[f"{prefix}{k}"] = v


def _note(out, form, label, role, ratio):
    M._note(form, role, ratio)
    out[label] = ratio


def _guard(label, fn):
    try:
        return fn()
    except AssertionError as e:
        if FAILS is None:
            raise AssertionError(f"stage {label}: {e}") from None
        FAILS.append(f"stage {label}: {e}")
        return 0.0


def _must(label, cond, msg):
    def f():
        assert cond, msg
    _guard(label, f)


def _rows_of_chunk(t, W, rank, j, c):
    """This rank's rows of chunk j's [Tc, ...] rows."""
    n = t.shape[0] // W
    return t[rank * n:(rank + 1) * n]


def _norm_dw_tp(role, allr, li, rank, cs, form):
    """A layer norm's weight gradient under sequence parallelism (see the module docstring)."""
    W = len(allr)
    key = {"dw1": ("dh1", "x", "rstd1", "dz", "w1"), "dw2": ("dh2", "z", "rstd2", "dout", "w2")}[role]
    me = allr[rank]["layers"][li]["s"][role]
    dw = torch.zeros(cs.w1.shape[0], dtype=F64)
    err, mass, locals_ = torch.zeros_like(dw), torch.zeros_like(dw), []
    for q in range(W):
        s = allr[q]["layers"][li]["s"]
        f = R.ref_norm_bwd(M.parts_bf16(s[key[0]]), s[key[1]], getattr(cs, key[4]), s[key[2]], s[key[3]], cs.mode)
        dw, err, mass = dw + f["dw"], err + f["dw_err"], mass + f["dw"].abs()
        locals_.append(s[role]["local"])
        if q == rank:   # this rank's own f32 column sum, before the sum over the group
            t, b = R.dw_target_bound(f["dw"], f["dw_err"], R.PT_DW_ACC_F32, torch.zeros_like(me["local"]))
            R.check(f"{role} (this rank's rows)", me["local"], t, b, form)
    res = {"sum": check_sum(f"{role} (f32 sum over tp)", me["tot"], locals_, form)}
    t, b = R.dw_target_bound(dw, err + (W - 1) * 2.0 ** -24 * mass, me["sink"], me.get("old"))
    want = F32 if me["sink"] == R.PT_DW_ACC_F32 else BF
    assert me["got"].dtype == want, f"{role}: dtype {me['got'].dtype}, the sink holds {want}"
    res["dw"] = R.check(role, me["got"], t, b, form)
    for q in range(W):
        R.check_exact(f"{role} (the same bits on rank {q})", allr[q]["layers"][li]["s"][role]["got"], me["got"])
    return res


def check_layer_tp(allr, li, rank, cs, cc, form, out):
    """Every stage of layer li on rank `rank`.  cs / cc: the layer constants with the shard's / one chunk's shape."""
    me = allr[rank]
    W, c, sp = me["W"], me["c"], me["sp"]
    L = me["layers"][li]
    s, ch = L["s"], L["ch"]
    every = [a["layers"][li] for a in allr]
    p = f"L{li} "
    cs0 = types.SimpleNamespace(**{**vars(cs), "w1_grad": not sp and cs.w1_grad, "w2_grad": not sp and cs.w2_grad})

    def mine(t, j):   # this rank's rows of chunk j's rows (replicated form: every row)
        return _rows_of_chunk(t, W, rank, j, c) if sp else t

    def srows(t, j):  # chunk j's rows of this rank's shard rows
        n = t.shape[0] // c
        return t[j * n:(j + 1) * n]

    def gathered(role, src, label):
        if sp:
            full = torch.cat([x[role] for x in ch])
            _note(out, form, p + label, label, _guard(p + label, lambda: check_layout(
                label, full, [e["s"][src] for e in every], c, form)))
        else:
            _note(out, form, p + label, label, _guard(p + label, lambda: R.check_exact(label, ch[0][role], s[src])))

    def summed(role, src, label):
        worst = 0.0
        for j in range(c):
            parts = [mine(e["ch"][j][src], j) for e in every]
            worst = max(worst, _guard(p + label, lambda: check_sum(f"{label} (chunk {j})", srows(s[role], j), parts, form)))
        _note(out, form, p + label, label, worst)

    _run(out, p, s, cs0, _stages(("h1",)), form)
    gathered("h1", "h1", "h1 gather")
    for j in range(c):
        _run(out, f"{p}c{j} ", ch[j], cc, _stages(CHUNK_ATTN_FWD), form)
    summed("a", "a", "ar")
    _run(out, p, s, cs0, _stages(("z",)), form)
    gathered("h2", "h2", "h2 gather")
    for j in range(c):
        _run(out, f"{p}c{j} ", ch[j], cc, _stages(CHUNK_MLP_FWD) + [M.Stage("m", "hh", _s_m)], form)
        _must(p + "m", (ch[j].get("m_res") is not None) == ((not sp) and rank == 0),
              f"m: the residual enters the tp sum from rank 0 only (rank {rank}: {ch[j].get('m_res') is not None})")
    if sp:
        summed("mr", "m", "mr")
        z = (s["z"].to(F64) + s["mr"].to(F64)).to(F32).to(BF)
        _note(out, form, p + "out", "out", _guard(p + "out", lambda: R.check_exact("out", s["out"], z)))
    else:
        summed("out", "m", "out")
    if "dout" not in s:
        return
    # ---- backward
    gathered("dout", "dout", "dm gather")
    for j in range(c):
        _run(out, f"{p}c{j} ", ch[j], cc, _stages(CHUNK_MLP_BWD), form)
    summed("dh2", "dh2", "dh2 sum")
    _run(out, p, s, cs0, _stages(("dz",)), form)
    gathered("dz", "dz", "da gather")
    for j in range(c):
        _run(out, f"{p}c{j} ", ch[j], cc, _stages(CHUNK_ATTN_BWD), form)
    summed("dh1", "dh1", "dh1 sum")
    _run(out, p, s, cs0, _stages(("dx",)), form)
    if sp:
        for role in ("dw1", "dw2"):
            _note(out, form, p + role, role, _guard(p + role, lambda: _norm_dw_tp(role, allr, li, rank, cs, form)))


def _ce_parts(h, hc, form):
    """This rank's 16-byte parts (max, sum-exp, target logit, own) against its logits shard."""
    x, tgt, part = h["logits"], h["targets"], h["part"]
    lo, Vs = h["vocab_lo"], h["logits"].shape[1]
    rows = torch.arange(x.shape[0])
    own = (tgt >= lo) & (tgt < lo + Vs)
    R.check_exact("ce parts (own: the rank whose slice holds the target)", part[:, 3], own.to(F32))
    xt = torch.where(own, x.to(F32)[rows, (tgt - lo).clamp(0, Vs - 1)], torch.zeros(x.shape[0]))
    R.check_exact("ce parts (target logit)", part[:, 2], xt)
    R.check_exact("ce parts (max)", part[:, 0], x.to(F32).amax(1))
    st = h["stats"].to(F64)
    _, merr = R.merge_stats(st[..., 0].t(), st[..., 1].t())
    f = R.ref_ce_fwd(x, torch.zeros_like(tgt), hc.ignore, steps=1)
    got = part[:, 0].to(F64) + torch.log(part[:, 1].to(F64))
    return R.check("ce parts (max + log sum-exp)", got, f["lse"], merr + f["lse_bound"], form)


def check_head_tp(allr, rank, hc, form, out):
    """The entry, the exit and the head on rank `rank`.  hc: head constants with this rank's shards (wlm, wemb)."""
    me = allr[rank]
    W, c, sp, h = me["W"], me["c"], me["sp"], me["head"]
    first, last = [a["layers"][0]["s"] for a in allr], [a["layers"][-1]["s"] for a in allr]
    lo_e = rank * hc.wemb.shape[0]

    def step(label, fn, role=None):
        _note(out, form, label, role or label, _guard(label, fn))

    # ---- entry: the masked lookup, its sum onto the shards
    step("x0", lambda: R.check_exact("x0 (masked lookup)", h["x0"], OR.emu_embedding_fwd(h["ids"], hc.wemb, lo_e, lo_e + hc.wemb.shape[0])))
    T = h["x0"].shape[0]
    cut = (lambda t: my_rows(t, W, rank, c)) if sp else (lambda t: t)
    step("x0 sum", lambda: check_sum("x0 sum", first[rank]["x"], [cut(a["head"]["x0"]) for a in allr], form))
    table = torch.cat([a["head"]["wemb"] for a in allr])
    step("x0 table", lambda: R.check_exact("x0 (the table's rows)", first[rank]["x"], cut(table[h["ids"].reshape(-1)])))
    # ---- exit and final norm
    if sp:
        step("xf gather", lambda: check_layout("xf", h["xf"], [e["out"] for e in last], c, form))
    else:
        step("xf gather", lambda: R.check_exact("xf", h["xf"], last[rank]["out"]))
    _run(out, "", h, hc, [s for s in M.HEAD_FWD if s.produces[0] in ("hf", "logits")], form)
    # ---- cross-entropy
    full = dict(h)
    full["logits"] = torch.cat([a["head"]["logits"] for a in allr], 1)
    Vs = h["logits"].shape[1]
    lo = rank * Vs
    if h.get("part") is not None:
        _must("ce parts", h["vocab_lo"] == lo, f"vocab_lo {h['vocab_lo']}, rank {rank}'s slice starts at {lo}")
        step("ce parts", lambda: _ce_parts(h, hc, form))
        full["stats"] = torch.cat([a["head"]["stats"] for a in allr], 0)
        for q, a in enumerate(allr):
            _guard("ce parts", lambda: R.check_exact(f"ce parts (gathered, rank {q}'s)", h["parts"][q], a["head"]["part"]))
    else:
        step("logits gather", lambda: R.check_exact("logits (gathered columns)", h["logits_full"], full["logits"]))
        full["stats"] = None
    _run(out, "", full, hc, [s for s in M.CE_STAGES if s.produces[0] in ("row_lse", "loss")], form)
    if "dlogits" not in h:
        return
    _run(out, "", full, hc, [s for s in M.CE_STAGES if s.produces[0] == "ce_scale"], form)

    def dlogits():
        tgt = full["targets"]
        rows = tgt.numel()
        gs = full["ce_scale"].to(F64).reshape(-1).expand(rows)
        ref, bound = R.ref_ce_bwd(full["logits"], tgt, full["row_lse"].to(F64), torch.zeros(rows, dtype=F64), gs, hc.ignore,
                                  style="fma")
        ign = tgt == hc.ignore
        if h.get("dlogits_full") is not None:   # the gathered-logits path: the whole gradient, then this rank's columns
            R.check_exact("dlogits (ignored rows)", h["dlogits_full"][ign], torch.zeros(int(ign.sum()), ref.shape[1], dtype=BF))
            w = R.check("dlogits", h["dlogits_full"], ref, bound, form)
            R.check_exact("dlogits (this rank's columns)", h["dlogits"], h["dlogits_full"][:, lo:lo + Vs])
            return w
        R.check_exact("dlogits (ignored rows)", h["dlogits"][ign], torch.zeros(int(ign.sum()), Vs, dtype=BF))
        return R.check("dlogits", h["dlogits"], ref[:, lo:lo + Vs], bound[:, lo:lo + Vs], form)
    step("dlogits", dlogits)
    # ---- lm_head backward: this rank's partial dX, its sum, the final norm (replicated: no sum over tp)
    hp = dict(h, dhf=h["dhf_part"])
    _run(out, "", hp, hc, [s for s in M.HEAD_BWD if s.produces[0] in ("dhf", "dW_lm")], form)
    step("dhf sum", lambda: check_sum("dhf sum", h["dhf"], [a["head"]["dhf_part"] for a in allr], form))
    _run(out, "", h, hc, [s for s in M.HEAD_BWD if s.produces[0] == "dxf"], form)
    _must("dxf/dwf", not h["dwf_collectives"], f"dwf: a collective touches the final norm's weight gradient ({h['dwf_collectives']})")
    if sp:
        step("dout shard", lambda: R.check_exact("dout (this rank's rows of dxf)", last[rank]["dout"], my_rows(h["dxf"], W, rank, c)))
        step("dx0 gather", lambda: check_layout("dx0", h["dx0"], [e["dx"] for e in first], c, form))
    else:
        step("dout shard", lambda: R.check_exact("dout", last[rank]["dout"], h["dxf"]))
        step("dx0 gather", lambda: R.check_exact("dx0", h["dx0"], first[rank]["dx"]))
    s = h["dW_emb"]
    step("dW_emb", lambda: R.check_exact("dW_emb", s["got"], OR.emu_embedding_bwd(
        h["ids"].reshape(-1), h["dx0"], s["old"], s["sink"], lo_e, lo_e + hc.wemb.shape[0])))


def check_tp(allr, rank, cfgs, hc, form, keep_going=False):
    """Every stage of rank `rank` from every rank's roles.  cfgs: [(shard constants, chunk constants)] per layer.
    Returns {label: worst ratio}; keep_going: (that, [the failing stages' messages]) instead of raising at the first."""
    global FAILS
    FAILS = [] if keep_going else None
    try:
        out = {}
        for li, (cs, cc) in enumerate(cfgs):
            check_layer_tp(allr, li, rank, cs, cc, form, out)
            if li:   # the data flow between the layers, by bits
                R.check_exact(f"layer {li}: x is the previous layer's out", allr[rank]["layers"][li]["s"]["x"],
                              allr[rank]["layers"][li - 1]["s"]["out"])
                if "dout" in allr[rank]["layers"][li]["s"]:
                    R.check_exact(f"layer {li - 1}: dout is the next layer's dx", allr[rank]["layers"][li - 1]["s"]["dout"],
                                  allr[rank]["layers"][li]["s"]["dx"])
        check_head_tp(allr, rank, hc, form, out)
        fails = FAILS
    finally:
        FAILS = None
    if OVER:
        msg, n = OVER[0], len(OVER)
        del OVER[:]
        if not keep_going:
            raise AssertionError(f"stage sums: {n} sums over their bound; the first: {msg}")
        fails.append(f"stage sums: {msg}")
    return (out, fails) if keep_going else out


# ============================================================================== extraction from a recorded trace
def _index(calls, call):
    return next(i for i, c in enumerate(calls) if c is call)


def _sp_norm_dw(calls, nb, sinks, name, role):
    """The chain of a sequence-parallel norm's weight gradient behind the backward call nb: the column sum of its
    partial rows into one f32 row (local), the all-reduce of the block that holds the row (tot), the sum of that one
    row into the sink (got, old, sink)."""
    part, at = nb.result[1], _index(calls, nb)
    assert nb.kwargs.get("defer_dw") and part is not None, f"role {role!r}: the norm backward left no partial rows"
    row = ar = None
    for i in range(at, len(calls)):
        c = calls[i]
        if row is None and c.name == "rmsnorm_colsum_batch":
            row = next((o for p, o, _ in c.arg(0) if p.same(part)), None)
        elif row is not None and ar is None and is_coll(c) and c.name == "all_reduce" and _overlap(extent(c.ins[0]), extent(row)):
            ar = c
            j = (row.key[0] - c.ins[0].key[0]) // (row.key[1][-1] * 4)
            assert cpu(c.ins[0].pre)[j].equal(cpu(row.post)), f"role {role!r}: the all-reduce's block does not hold the column sum"
        elif ar is not None and c.name == "rmsnorm_colsum_batch":
            for p, o, sink in c.arg(0):
                if p.key[0] == row.key[0] and sinks.get(o.key[0]) == name:
                    return dict(local=cpu(row.post), tot=cpu(ar.outs[0].post)[j], got=cpu(o.post), old=cpu(o.pre), sink=sink,
                                at=(at, i))
    raise AssertionError(f"role {role!r}: no recorded call produces it (partial rows -> f32 row -> all-reduce -> {name})")


def extract_tp(K, calls, model, B, S, gloss, W, rank, c, sp):
    """Every role of one forward + backward of a tensor-parallel Llama on this rank (see the module docstring), the
    layers' and the head's constants: (roles, [(shard constants, chunk constants)], head constants)."""
    T = B * S
    sinks = M.grad_sinks(model)
    wev, nev = M.sink_events(calls, sinks), M.norm_sink_events(calls, sinks)
    cur = M.Cursor(calls, 0)
    h = {}
    ec = cur.next("embedding_fwd", None, "x0")
    h["ids"], h["x0"], h["wemb"] = cpu(ec.arg(0).pre), cpu(ec.result.post).reshape(T, -1), cpu(model.embedding.weight)
    layers, cfgs = [], []
    nc = c if sp else 1
    for i, layer in enumerate(model.decoder_layers):
        cs = M.layer_config(layer, B, S // W if sp else S)
        cc = M.layer_config(layer, B // nc, S)
        s, ch = {}, [{} for _ in range(nc)]
        n1 = cur.next("rmsnorm_fwd", lambda k: M._is(k.arg(1), layer.input_layernorm.weight) and k.kwargs.get("residual") is None, "h1")
        s["x"], s["h1"], s["rstd1"] = cpu(n1.arg(0).pre), cpu(n1.result[0].post), cpu(n1.result[1].post)
        for j in range(nc):
            qc = M.extract_attn_fwd(K, layer, cur, cc, ch[j], None)
            ch[j]["h1"] = cpu(qc.arg(0).pre)
        n2 = cur.next("rmsnorm_fwd", lambda k: M._is(k.arg(1), layer.post_attention_layernorm.weight) and
                      k.kwargs.get("residual") is not None, "h2")
        s["a"] = cpu(n2.arg(0).pre)
        s["h2"], s["rstd2"], s["z"] = (cpu(t.post) for t in n2.result)
        M._bits_equal(f"layer {i}: the fused norm's residual is x", n2.kwargs["residual"].pre, n1.arg(0).pre)
        for j in range(nc):
            gc, dc = M.extract_mlp_fwd(K, layer, cur, cc, ch[j], None, residual=None)
            ch[j]["h2"], ch[j]["m"] = cpu(gc.arg(0).pre), ch[j].pop("out")
            res = dc.kwargs.get("residual")
            ch[j]["m_res"] = cpu(res.pre) if res is not None else None
            if res is not None:
                M._bits_equal(f"layer {i}: the down projection's residual is z", res.pre, n2.result[2].post)
        if sp:
            ra = cur.next("residual_add", None, "out")
            s["mr"], s["out"] = cpu(ra.arg(1).pre), cpu(ra.result.post)
            M._bits_equal(f"layer {i}: the residual add reads z", ra.arg(0).pre, n2.result[2].post)
        else:
            ac = cur.next("all_reduce", None, "out")
            s["out"] = cpu(ac.outs[0].post)
        layers.append(dict(s=s, ch=ch))
        cfgs.append((cs, cc))
    # ---- head forward
    hc = M.head_config(model)
    fc = cur.next("rmsnorm_fwd", lambda k: M._is(k.arg(1), model.final_norm.weight), "hf")
    h["xf"], h["hf"], h["rstdf"] = cpu(fc.arg(0).pre), cpu(fc.result[0].post), cpu(fc.result[1].post)
    lc = cur.next(("linear_ce_stats", "linear_fwd"),
                  lambda k: M._is(k.arg(1), model.final_proj.weight) or M._is(M._first_weight(k), model.final_proj.weight), "logits")
    if lc.name == "linear_ce_stats":
        with M.single_pass():
            plain = K.linear_fwd(fc.result[0].post, [model.final_proj.weight])
        M._bits_equal("logits: linear_ce_stats vs linear_fwd", lc.result[0].post, plain)
        h["logits"], h["stats"] = cpu(lc.result[0].post), cpu(lc.result[1].post)
        pc = cur.next("cross_entropy_vp_partial", None, "ce parts")
        M._bits_equal("the CE's logits are the lm_head's", pc.arg(0).pre, lc.result[0].post)
        M._bits_equal("the CE's statistics are the lm_head's", pc.arg(2).pre, lc.result[1].post)
        h["targets"], h["part"], h["vocab_lo"] = cpu(pc.arg(1).pre), cpu(pc.result.post), int(pc.arg(3))
        cb = cur.next("cross_entropy_vp_combine", None, "row_lse")
        h["parts"] = cpu(cb.arg(0).pre)
        h["loss"], h["inv_count"], h["row_lse"] = cpu(cb.result[0].post), cpu(cb.result[1].post), cpu(cb.result[2].post)
        bc = cur.next("cross_entropy_grad_lse_shard", None, "dlogits")
        M._bits_equal("the backward's logits are the forward's", bc.arg(0).pre, lc.result[0].post)
        M._bits_equal("the backward's row_lse is the forward's", bc.arg(2).pre, cb.result[2].post)
        assert int(bc.arg(4)) == h["vocab_lo"], f"stage dlogits: vocab_lo {bc.arg(4)} in the backward, {h['vocab_lo']} in the forward"
        h["gloss"], h["ce_scale"], h["dlogits"] = cpu(gloss), cpu(bc.arg(3).pre), cpu(bc.result.post)
        ce_name = "cross_entropy_vp_combine"
    else:
        h["logits"] = cpu(lc.result.post)
        ce, ce_name, cur = M.extract_ce(K, calls, cur.at, gloss)
        h["logits_full"], h["dlogits_full"] = ce.pop("logits"), ce.pop("dlogits")
        h.update({k: v for k, v in ce.items() if not k.startswith("_")})
    start = cur.at
    dc = cur.next("linear_dgrad", lambda k: M._is(M._first_weight(k), model.final_proj.weight), "dhf")
    if "dlogits" not in h:
        h["dlogits"] = cpu(dc.arg(0).pre)
    h["dhf_part"] = cpu(dc.result.post)
    h["dW_lm"] = M._sink_role(M._wsink(wev, "final_proj.weight", start, "dW_lm"))
    nb = cur.next("rmsnorm_bwd", lambda k: M._is(k.arg(2), model.final_norm.weight), "dxf")
    h["dhf"], h["dxf"] = cpu(nb.arg(0).pre), cpu(nb.result[0].post)
    part = nb.result[1] if nb.kwargs.get("defer_dw") else None
    h["dwf"] = M._norm_sink(nev, "final_norm.weight", part, start, "dwf")
    ev = next(e for e in nev["final_norm.weight"] if e["call"] >= start)
    g = getattr(model.final_norm.weight, "main_grad", None)
    g = model.final_norm.weight.grad if g is None else g
    watch = [(g.data_ptr(), g.data_ptr() + g.numel() * g.element_size())] + ([extent(part)] if part is not None else [])
    h["dwf_collectives"] = [f"{k.name} at call {i}" for i, k in enumerate(calls) if is_coll(k) and
                            any(_overlap(extent(r), w) for r in k.ins + k.outs
                                for w in (watch if _index(calls, nb) <= i <= ev["call"] else watch[:1]))]
    # ---- layers backward
    for i in reversed(range(len(layers))):
        layer, names = model.decoder_layers[i], M.layer_names(model, i)
        s, ch = layers[i]["s"], layers[i]["ch"]
        cs, cc = cfgs[i]
        for j in range(nc):
            M.extract_mlp_bwd(K, layer, names, cur, cc, ch[j], wev)
        st = cur.at
        n2 = cur.next("rmsnorm_bwd", lambda k: M._is(k.arg(2), layer.post_attention_layernorm.weight), "dz")
        s["dh2"], s["dout"], s["dz"] = cpu(n2.arg(0).pre), cpu(n2.kwargs["dres"].pre), cpu(n2.result[0].post)
        if sp:
            s["dw2"] = _sp_norm_dw(calls, n2, sinks, names["w2"], "dw2")
        elif cs.w2_grad:
            s["dw2"] = M._norm_sink(nev, names["w2"], n2.result[1] if n2.kwargs.get("defer_dw") else None, st, "dw2")
        for j in range(nc):
            M.extract_attn_bwd(K, layer, names, cur, cc, ch[j], wev, nev)
        st = cur.at
        n1 = cur.next("rmsnorm_bwd", lambda k: M._is(k.arg(2), layer.input_layernorm.weight), "dx")
        s["dh1"], s["dx"] = cpu(n1.arg(0).pre), cpu(n1.result[0].post)
        M._bits_equal(f"layer {i}: the input norm's residual gradient is dz", n1.kwargs["dres"].pre, n2.result[0].post)
        if sp:
            s["dw1"] = _sp_norm_dw(calls, n1, sinks, names["w1"], "dw1")
        elif cs.w1_grad:
            s["dw1"] = M._norm_sink(nev, names["w1"], n1.result[1] if n1.kwargs.get("defer_dw") else None, st, "dw1")
        # chunk j's weight-gradient launch is the j-th into its sink (a block's dW launches follow its dX, so the
        # first event behind the block's start is not the block's own): by index, and its dY must be the chunk's
        for nm, role, dy in (("wd", "dW_d", "dout"), ("wg", "dW_g", "dgu"), ("wu", "dW_u", "dgu"), ("wo", "dW_o", "dz"),
                             ("wq", "dW_q", "dqkv"), ("wk", "dW_k", "dqkv"), ("wv", "dW_v", "dqkv")):
            evs = wev.get(names[nm], [])
            assert len(evs) == nc, f"role {role!r}: {len(evs)} weight-gradient launches into {names[nm]} for {nc} chunks"
            for j, e in enumerate(evs):
                ch[j][role] = M._sink_role(e)
                if tuple(e["dy"].key[1]) == tuple(ch[j][dy].shape):
                    M._bits_equal(f"layer {i} chunk {j}: the dY of the launch into {names[nm]} is the chunk's {dy}", e["dy"].pre, ch[j][dy])
    eb = cur.next("embedding_bwd", None, "dW_emb")
    h["dx0"] = cpu(eb.arg(1).pre)
    h["dW_emb"] = dict(got=cpu(eb.arg(2).post), old=cpu(eb.arg(2).pre), sink=eb.arg(3))
    hc.wemb = h["wemb"]
    roles = dict(W=W, rank=rank, c=nc, sp=sp, layers=layers, head=h)
    return roles, cfgs, hc, ce_name, (wev, nev)


def check_notifications(calls, wev, nev, sp):
    """The owner of a gradient is told exactly once, after the last launch into its sink (a chunked layer: the
    last chunk's); a norm weight summed over tp after its store.  Returns {name: launches}."""
    told = {}
    for i, k in enumerate(calls):
        if k.name == "grad_ready":
            told.setdefault(k.param, []).append(i)
    out = {}
    for name, evs in list(wev.items()) + [(n, e) for n, e in nev.items() if sp and "final_norm" not in n]:
        at = told.get(name, [])
        assert len(at) == 1, f"notification: the owner of {name} is told {len(at)} times for {len(evs)} launches"
        assert at[0] > evs[-1]["call"], f"notification: the owner of {name} is told before the last launch into its sink"
        out[name] = len(evs)
    for name, at in told.items():
        assert len(at) <= 1, f"notification: the owner of {name} is told {len(at)} times"
    return out


def _strip(x):
    if isinstance(x, dict):
        return {k: _strip(v) for k, v in x.items() if not (isinstance(k, str) and (k.startswith("_") or k.startswith("dW_")))}
    if isinstance(x, list):
        return [_strip(v) for v in x]
    return x


def exchange(roles, group=None):
    """Every rank's roles (CPU tensors; the weight-gradient sinks stay at home), this rank's own entry whole."""
    import torch.distributed as dist
    W = roles["W"]
    out = [None] * W
    dist.all_gather_object(out, _strip(roles), group=group)
    out[roles["rank"]] = roles
    return out


# ============================================================================== CPU emulation of W ranks
FAULTS = ("residual_on_every_rank", "gather_slot_rotated", "h2_chunk_stale", "scatter_other_ranks_rows", "partial_missing",
          "norm_dw_not_summed", "final_dw_summed", "chunk_store_for_accumulate", "own_on_non_owner", "dlogits_next_vocab_lo",
          "embedding_out_of_slice_nonzero", "consumer_before_wait", "handle_never_waited")
# fault -> (the form it is injected into: (W, c, sp), the stage label that must reject it, a word of its message)
FAULT_ROLE = {
    "residual_on_every_rank": ((2, 1, False), "L0 m", "rank 0 only"),
    "gather_slot_rotated": ((2, 2, True), "L0 h1 gather", "h1"),
    "h2_chunk_stale": ((2, 2, True), "L0 h2 gather", "h2"),
    "scatter_other_ranks_rows": ((2, 2, True), "L0 ar", "ar (chunk 1)"),
    "partial_missing": ((2, 2, True), "L0 mr", "mr"),
    "norm_dw_not_summed": ((2, 2, True), "L0 dw2", "dw2"),
    "final_dw_summed": ((2, 2, True), "dxf/dwf", "dwf"),
    "chunk_store_for_accumulate": ((2, 2, True), "L0 c1 dW_d", "dW_d"),
    "own_on_non_owner": ((2, 2, True), "ce parts", "own"),
    "dlogits_next_vocab_lo": ((2, 2, True), "dlogits", "dlogits"),
    "embedding_out_of_slice_nonzero": ((2, 2, True), "x0", "x0"),
    "consumer_before_wait": ((2, 2, True), "wait ledger", "not yet waited"),
    "handle_never_waited": ((2, 2, True), "wait ledger", "waited"),   # (its consumer then runs unwaited, or the node returns)
}


def emu_shard(c, W, q, B):
    """Rank q's constants of the full emulated model c (tests/_model_ref.emu_config): Column shards are row blocks,
    Row shards column blocks, the vocabulary in W slices."""
    blk = lambda w, dim: w.chunk(W, dim)[q].contiguous()   # noqa: E731
    return types.SimpleNamespace(**{
        **vars(c), "B": B, "nh": c.nh // W, "nkv": c.nkv // W, "I": c.I // W, "wq": blk(c.wq, 0), "wk": blk(c.wk, 0),
        "wv": blk(c.wv, 0), "wo": blk(c.wo, 1), "wg": blk(c.wg, 0), "wu": blk(c.wu, 0), "wd": blk(c.wd, 1),
        "wlm": blk(c.wlm, 0), "wemb": blk(c.wemb, 0)})


def _sum(parts):
    return sum(p.to(F64) for p in parts).to(F32).to(parts[0].dtype)


def _dw_sink(c, dw32, sink):
    """A norm weight-gradient role: the f32 column sum dw32 into a sink with prior contents."""
    old = M._old(c, tuple(dw32.shape), F32 if sink == R.PT_DW_ACC_F32 else BF)
    if sink == R.PT_DW_ACC_F32:
        got = old + dw32
    else:
        got = (old.to(F32) + dw32.to(BF).to(F32)).to(BF)
    return dict(got=got, old=old, sink=sink)


def emu_tp(c, W, nc, sp, fault=None):
    """Every rank's roles of embedding -> one decoder layer -> final norm -> vocab-parallel lm_head and CE, forward and
    backward, W ranks in one process: shard weights, the partials summed here in the documented layout.  Returns
    (roles per rank, [(shard constants, chunk constants)] per rank, head constants per rank)."""
    assert fault is None or fault in FAULTS, fault
    from tests import _attn_ref as A
    T, H, Wr = c.B * c.S, c.w1.shape[0], range(W)
    nc = nc if sp else 1
    Tc = T // nc
    cc = [emu_shard(c, W, q, c.B // nc) for q in Wr]
    cut = (lambda t, q: my_rows(t, W, q, nc)) if sp else (lambda t, q: t)
    full = (lambda shards: layout(shards, nc)) if sp else (lambda shards: shards[0])
    S_, CH, Hd = [dict() for _ in Wr], [[dict() for _ in range(nc)] for _ in Wr], [dict() for _ in Wr]
    Vs = c.wlm.shape[0] // W
    ids = c.ids.reshape(-1)
    # ---- entry
    for q in Wr:
        h = Hd[q]
        h["ids"], h["wemb"] = c.ids, cc[q].wemb
        h["x0"] = OR.emu_embedding_fwd(ids, cc[q].wemb, q * Vs, (q + 1) * Vs)
        if fault == "embedding_out_of_slice_nonzero" and q == 1:
            row = int((ids < Vs).nonzero()[0])
            h["x0"][row] = cc[q].wemb[0]
    for q in Wr:
        S_[q]["x"] = cut(_sum([Hd[p]["x0"] for p in Wr]), q)

    def gather(role, src, rot=False, stale=False):
        for q in Wr:
            shards = [S_[p][src] for p in Wr]
            if rot:
                shards = shards[-1:] + shards[:-1]
            g = full(shards).clone()
            if stale and q == 0:
                g[Tc:2 * Tc] = g[:Tc]
            for j in range(nc):
                CH[q][j][role] = g[j * Tc:(j + 1) * Tc]

    def scatter(role, src, other=False, missing=False):
        for q in Wr:
            rows = []
            for j in range(nc):
                parts = [_rows_of_chunk(CH[p][j][src], W, q, j, nc) if sp else CH[p][j][src] for p in Wr]
                if other and q == 0 and j == 1:
                    parts = [_rows_of_chunk(CH[p][j][src], W, 1, j, nc) for p in Wr]
                if missing and j == 0:
                    parts = parts[:1] + [torch.zeros_like(parts[0])] * (W - 1)
                rows.append(_sum(parts))
            S_[q][role] = torch.cat(rows)

    # ---- layer forward
    for q in Wr:
        s = S_[q]
        s["h1"], _, s["rstd1"] = R.emu_norm_fwd(s["x"], None, c.w1, c.eps, c.mode)
    gather("h1", "h1", rot=fault == "gather_slot_rotated")
    sc = A.scale_of(c.d)
    for q in Wr:
        k = cc[q]
        wqkv = torch.cat([k.wq, k.wk, k.wv])
        for r in CH[q]:
            r["qkv_raw"] = G.emu_gemm(r["h1"], wqkv.t().contiguous(), G.EPI_BF16)
            r["qkv"] = R.emu_rope(r["qkv_raw"], k.nh + k.nkv, k.d, k.cos, k.sin, k.S)
            r["o"], r["lse"] = A.emu_forward(*(M._heads(r["qkv"], k, n) for n in "qkv"), sc, True)
            r["a"] = G.emu_gemm(r["o"].reshape(Tc, -1), k.wo.t().contiguous(), G.EPI_BF16)
    scatter("a", "a", other=fault == "scatter_other_ranks_rows")
    for q in Wr:
        s = S_[q]
        s["h2"], s["z"], s["rstd2"] = R.emu_norm_fwd(s["a"], s["x"], c.w2, c.eps, c.mode)
    gather("h2", "h2", stale=fault == "h2_chunk_stale")
    for q in Wr:
        k = cc[q]
        wgu = torch.cat([k.wg, k.wu])
        for r in CH[q]:
            r["gu"] = G.emu_gemm(r["h2"], wgu.t().contiguous(), G.EPI_BF16)
            r["hh"] = R.emu_swiglu(r["gu"][:, :k.I], r["gu"][:, k.I:], torch.zeros_like(r["gu"][:, :k.I]))[0]
            res = S_[q]["z"] if not sp and (q == 0 or fault == "residual_on_every_rank") else None
            r["m_res"] = res
            r["m"] = G.emu_gemm(r["hh"], k.wd.t().contiguous(), G.EPI_BF16_RES if res is not None else G.EPI_BF16, residual=res)
    scatter("mr" if sp else "out", "m", missing=fault == "partial_missing")
    if sp:
        for s in S_:
            s["out"] = (s["z"].to(F64) + s["mr"].to(F64)).to(F32).to(BF)
    # ---- head forward: exit gather, final norm, the vocab shard's logits, the CE from the 16-byte parts
    tgt = c.targets.clone()
    tgt[::19] = c.ignore
    valid = tgt != c.ignore
    for q in Wr:
        h = Hd[q]
        h["xf"] = full([S_[p]["out"] for p in Wr])
        h["hf"], _, h["rstdf"] = R.emu_norm_fwd(h["xf"], None, c.wf, c.eps, c.mode)
        x = h["logits"] = G.emu_gemm(h["hf"], cc[q].wlm.t().contiguous(), G.EPI_BF16)
        tiles = x.to(F32).reshape(T, Vs // 128, 128)
        mx = tiles.amax(2)
        h["stats"] = torch.stack([mx, torch.exp(tiles - mx[..., None]).sum(2)], -1).permute(1, 0, 2).contiguous()
        m = mx.amax(1)
        own = (tgt >= q * Vs) & (tgt < (q + 1) * Vs)
        if fault == "own_on_non_owner" and q == 1:
            own = own | (valid & (tgt < Vs) & (torch.arange(T) % 2 == 0))
        xt = torch.where(own, x.to(F32)[torch.arange(T), (tgt - q * Vs).clamp(0, Vs - 1)], torch.zeros(T))
        h["part"] = torch.stack([m, torch.exp(x.to(F32) - m[:, None]).sum(1), xt, own.to(F32)], 1)
        h["targets"], h["vocab_lo"] = tgt, q * Vs
    parts = torch.stack([Hd[q]["part"] for q in Wr])
    gm = parts[..., 0].amax(0)
    lse = gm + torch.log((parts[..., 1] * torch.exp(parts[..., 0] - gm)).sum(0))
    row_loss = torch.where(valid, lse - parts[..., 2].sum(0), torch.zeros(T))
    inv = torch.tensor([1.0], dtype=F32) / torch.tensor([float(valid.sum())], dtype=F32)
    gloss = torch.tensor(0.25, dtype=BF)
    for q in Wr:
        h = Hd[q]
        h["parts"], h["row_lse"], h["inv_count"], h["loss"] = parts, lse, inv, (row_loss.sum() * inv[0]).to(BF)
        h["gloss"], h["ce_scale"] = gloss, gloss.to(F32).reshape(1) * inv
        lo = ((q + 1) % W if fault == "dlogits_next_vocab_lo" else q) * Vs
        p = torch.exp(h["logits"].to(F32) - lse[:, None])
        onehot = (torch.arange(Vs)[None, :] == (tgt - lo)[:, None]).to(F32)
        g = torch.where(valid, h["ce_scale"].expand(T), torch.zeros(T))[:, None]
        h["dlogits"] = ((p - onehot) * g).to(BF)
        h["dhf_part"] = G.emu_gemm(h["dlogits"], cc[q].wlm, G.EPI_BF16)
        h["dW_lm"] = M._emu_sink(c, h["dlogits"], h["hf"], G.EPI_BF16_ACC)
    for q in Wr:
        h = Hd[q]
        h["dhf"] = _sum([Hd[p]["dhf_part"] for p in Wr])
        h["dxf"], dwf = R.emu_norm_bwd(h["dhf"], h["xf"], c.wf, h["rstdf"], None, c.mode, R.PT_DW_ACC_F32, torch.zeros(H))
        h["dwf"] = _dw_sink(c, dwf * (W if fault == "final_dw_summed" else 1), R.PT_DW_ACC_BF16)
        h["dwf_collectives"] = []
        S_[q]["dout"] = cut(h["dxf"], q)
    # ---- layer backward
    gather("dout", "dout")
    for q in Wr:
        k = cc[q]
        wgu = torch.cat([k.wg, k.wu])
        prev = {}
        for j, r in enumerate(CH[q]):
            r["dhh"] = G.emu_gemm(r["dout"], k.wd, G.EPI_BF16)
            _, dg, du = R.emu_swiglu(r["gu"][:, :k.I], r["gu"][:, k.I:], r["dhh"])
            r["dgu"] = torch.cat([dg, du], 1)
            r["dh2"] = G.emu_gemm(r["dgu"], wgu, G.EPI_BF16)
            for role, dy, x in (("dW_d", r["dout"], r["hh"]), ("dW_g", dg, r["h2"]), ("dW_u", du, r["h2"])):
                r[role] = _emu_chunk_sink(prev, role, dy, x, fault == "chunk_store_for_accumulate" and role == "dW_d" and j == 1)
    scatter("dh2", "dh2")
    _emu_norm_tp(c, S_, W, sp, "dw2", "dh2", "z", c.w2, "rstd2", "dout", "dz", fault == "norm_dw_not_summed")
    gather("dz", "dz")
    for q in Wr:
        k = cc[q]
        wqkv = torch.cat([k.wq, k.wk, k.wv])
        prev = {}
        for j, r in enumerate(CH[q]):
            r["do"] = G.emu_gemm(r["dz"], k.wo, G.EPI_BF16)
            qh, kh, vh = (M._heads(r["qkv"], k, n) for n in "qkv")
            dq, dk, dv, _ = A.emu_backward(qh, kh, vh, r["do"].reshape(k.B, k.S, k.nh, k.d), r["o"], r["lse"], sc, True)
            r["dqkv_unrot"] = torch.cat([t.reshape(Tc, -1) for t in (dq, dk, dv)], 1)
            r["dqkv_rot"] = r["dqkv"] = R.emu_rope(r["dqkv_unrot"], k.nh + k.nkv, k.d, k.cos, k.sin, k.S, inverse=True)
            r["dh1"] = G.emu_gemm(r["dqkv"], wqkv, G.EPI_BF16)
            r["dW_o"] = _emu_chunk_sink(prev, "dW_o", r["dz"], r["o"].reshape(Tc, -1), False)
            lo = 0
            for nm, w in (("q", k.wq), ("k", k.wk), ("v", k.wv)):
                r["dW_" + nm] = _emu_chunk_sink(prev, "dW_" + nm, r["dqkv"][:, lo:lo + w.shape[0]], r["h1"], False)
                lo += w.shape[0]
    scatter("dh1", "dh1")
    _emu_norm_tp(c, S_, W, sp, "dw1", "dh1", "x", c.w1, "rstd1", "dz", "dx", False)
    for q in Wr:
        h = Hd[q]
        h["dx0"] = full([S_[p]["dx"] for p in Wr])
        old = M._old(c, tuple(cc[q].wemb.shape), BF)
        h["dW_emb"] = dict(got=OR.emu_embedding_bwd(ids, h["dx0"], old, R.PT_DW_ACC_BF16, q * Vs, (q + 1) * Vs), old=old,
                           sink=R.PT_DW_ACC_BF16)
    allr = [dict(W=W, rank=q, c=nc, sp=sp, layers=[dict(s=S_[q], ch=CH[q])], head=Hd[q]) for q in Wr]
    cfgs = [[(emu_shard(c, W, q, c.B), cc[q])] for q in Wr]
    return allr, cfgs, cc


def _emu_chunk_sink(prev, role, dy, x, store):
    """Chunk j's weight-gradient event: chunk 0 stores into a fresh bf16 .grad, every later chunk accumulates onto
    the recorded prior contents (store: the fault -- the later chunk stores too)."""
    old = prev.get(role)
    epi = G.EPI_BF16 if old is None else G.EPI_BF16_ACC
    got = G.emu_gemm(dy.t().contiguous(), x.contiguous(), G.EPI_BF16 if store else epi, old=old)
    prev[role] = got
    return dict(got=got, old=old if old is not None else torch.zeros_like(got), epi=epi)


def _emu_norm_tp(c, S_, W, sp, role, dy, z, w, rstd, dres, dx, not_summed):
    """A layer norm's backward on every rank: dx, and the weight gradient -- sequence parallelism: this rank's f32
    column sum, the sum over the group, the sink; the replicated form: every rank's own."""
    locals_ = []
    for s in S_:
        s[dx], loc = R.emu_norm_bwd(s[dy], s[z], w, s[rstd], s[dres], c.mode, R.PT_DW_ACC_F32, torch.zeros(w.shape[0]))
        locals_.append(loc)
    tot = _sum(locals_)
    old = M._old(c, (w.shape[0],), BF)
    for q, s in enumerate(S_):
        t = locals_[q] if (not_summed or not sp) else tot
        got = (old.to(F32) + t.to(BF).to(F32)).to(BF)
        s[role] = dict(local=locals_[q], tot=t, got=got, old=old, sink=R.PT_DW_ACC_BF16)


# ------------------------------------------------------------------------------ the emulated trace (the ledger's input)
class EmuTrace:
    """The call and collective log of one rank's chunked sequence-parallel layer, forward and backward, in
    production's order (functional._forward_sp / _backward_sp) on small stand-in buffers: the ledger reads
    identities and order only."""

    def __init__(self, W, rank, c, fault=None):
        self.W, self.rank, self.c, self.fault, self.calls = W, rank, c, fault, []
        n, H = 4, 8
        self.n, self.Tc = n, n * W
        new = lambda rows: torch.zeros(rows, H, dtype=BF)   # noqa: E731
        for kind in ("fwd", "bwd"):
            x = new(c * n)
            order = ("attn", "mlp") if kind == "fwd" else ("mlp", "attn")
            for blk in order:
                shard = self.k("rmsnorm_" + kind, [x], [new(c * n)])
                x = self.block(blk, shard, new)
            self.k("residual_add" if kind == "fwd" else "rmsnorm_bwd", [x], [new(c * n)])
            ev = Call("node_end", (), {})
            ev.kind, ev.layer = kind, 0
            self.calls.append(ev)

    def k(self, name, reads, outs):
        call = Call(name, tuple(Rec(t, t) for t in reads), {})
        for r in call.args:
            r.post = r.pre
        call.result = tuple(Rec(t, None) for t in outs)
        for r in call.result:
            r.post = r.obj
        self.calls.append(call)
        return outs[0]

    def wait(self, coll):
        ev = Call("wait", (), {})
        ev.of = coll
        self.calls.append(ev)

    def issue(self, name, src, dst):
        call = coll_call(name, [Rec(src, src)], [Rec(dst, dst)], False, self.rank, self.W)
        self.calls.append(call)
        return call

    def block(self, blk, shard, new):
        """All-gather the shard chunk by chunk, run the block on each gathered chunk, reduce-scatter its output."""
        c, n, Tc = self.c, self.n, self.Tc
        fullb, outb = new(c * Tc), new(c * n)
        ag = [self.issue("all_gather_rows_into", shard[j * n:(j + 1) * n], fullb[j * Tc:(j + 1) * Tc]) for j in range(c)]
        rs = []
        for j in range(c):
            early = self.fault == "consumer_before_wait" and blk == "attn" and j == 1
            if not early:
                self.wait(ag[j])
            part = self.k(blk + "_block", [fullb[j * Tc:(j + 1) * Tc]], [new(Tc)])
            if early:
                self.wait(ag[j])
            rs.append(self.issue("reduce_scatter_rows_into", part, outb[j * n:(j + 1) * n]))
        for j, h in enumerate(rs):
            if not (self.fault == "handle_never_waited" and blk == "mlp" and j == 0):
                self.wait(h)
        return outb
