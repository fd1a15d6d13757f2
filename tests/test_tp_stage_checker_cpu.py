"""The tensor-parallel stage kit (tests/_tp_ref.py) tested on itself, without a GPU.

  * the emulation of W ranks in one process (shard weights, the partials summed in the documented token-row layout)
    passes every stage on every rank: W 2 in one and in two chunks, W 4, and the replicated stream;
  * every injected wiring fault is rejected at the stage where it was injected, on the ranks it touches, and the
    failure names that role; every other stage still passes on the faulty run's own values (teacher forcing: the
    fault does not travel), except where the faulty value IS another stage's output too (listed in ALSO);
  * the gathered-logits head (vp_ce = 0) passes, and rejects shards gathered in the wrong order and another
    rank's columns of the gradient;
  * the issue / wait ledger passes production's order of issue, consumer and wait, and rejects a consumer logged
    before its chunk's wait and a handle that is never waited;
  * the recorder of the collectives, over gloo-free stand-ins, logs issue and wait, returns a handle where the
    transport returned None, and keeps the identities the ledger works on.
"""
import pytest
import torch

from tests import _attn_ref as A
from tests import _gemm_ref as G
from tests import _model_ref as M
from tests import _row_ref as R
from tests import _tp_ref as T

BF, F32 = torch.bfloat16, torch.float32
# fault -> stages that fail beside the named one because the faulty value is their output as well
ALSO = {"embedding_out_of_slice_nonzero": ("x0 table",),   # the summed row is no longer the table's
        "own_on_non_owner": ("loss",)}                      # the target logit enters the loss twice


@pytest.fixture(autouse=True)
def _leave_the_worst_tables_alone():
    saved = [dict(t) for t in (M.WORST, G.WORST, R.WORST, A.WORST)]
    yield
    for t, s in zip((M.WORST, G.WORST, R.WORST, A.WORST), saved):
        t.clear()
        t.update(s)


def _config(W):
    return M.emu_config(B=2, V=512, nkv=4 if W == 4 else 2)


def _check_all(allr, cfgs, hcs, keep_going=False):
    return [T.check_tp(allr, q, cfgs[q], hcs[q], "emu", keep_going) for q in range(len(allr))]


@pytest.mark.parametrize("W,c,sp", [(2, 1, True), (2, 2, True), (4, 2, True), (2, 1, False)])
def test_clean_emulation_passes_every_stage_on_every_rank(W, c, sp):
    allr, cfgs, hcs = T.emu_tp(_config(W), W, c, sp)
    for res in _check_all(allr, cfgs, hcs):
        nc = c if sp else 1
        want = {f"L0 c{j} " + ("/".join(s.produces) or "dW_qkv") for j in range(nc)
                for s in T._stages(T.CHUNK_ATTN_FWD + T.CHUNK_MLP_FWD + T.CHUNK_MLP_BWD + T.CHUNK_ATTN_BWD)}
        want |= {f"L0 c{j} m" for j in range(nc)}
        want |= {"L0 " + k for k in ("h1/rstd1", "h1 gather", "ar", "z/h2/rstd2", "h2 gather", "out", "dm gather", "dh2 sum", "dz",
                                     "da gather", "dh1 sum", "dx")}
        want |= {"L0 mr", "L0 dw1", "L0 dw2"} if sp else set()
        want |= {"x0", "x0 sum", "x0 table", "xf gather", "hf/rstdf", "logits", "ce parts", "row_lse", "loss", "ce_scale",
                 "dlogits", "dhf", "dW_lm", "dhf sum", "dxf/dwf", "dout shard", "dx0 gather", "dW_emb"}
        assert set(res) == want, sorted(want ^ set(res))


@pytest.mark.parametrize("fault", [f for f in T.FAULTS if T.FAULT_ROLE[f][1] != "wait ledger"])
def test_fault_is_rejected_at_its_stage(fault):
    (W, c, sp), stage, word = T.FAULT_ROLE[fault]
    allr, cfgs, hcs = T.emu_tp(_config(W), W, c, sp, fault=fault)
    fails = [f for _, fs in _check_all(allr, cfgs, hcs, keep_going=True) for f in fs]
    assert fails, f"{fault}: no stage rejects it"
    named = [f for f in fails if f.split(": ")[0] == f"stage {stage}"]
    assert named and all(word in f for f in named), fails
    print(f"{fault}: {named[0][:170]}")
    for f in fails:   # nothing else fails: the fault does not travel
        assert f.split(": ")[0] in [f"stage {a}" for a in (stage,) + ALSO.get(fault, ())], f"{fault}: also rejected at {f[:200]}"


def _as_gathered_logits(allr):
    """The head roles of the gathered-logits path (vp_ce = 0): no parts, the CE on the column-concatenated logits."""
    full = torch.cat([a["head"]["logits"] for a in allr], 1)
    dfull = torch.cat([a["head"]["dlogits"] for a in allr], 1)
    for a in allr:
        h = a["head"]
        for k in ("part", "parts", "stats", "vocab_lo"):
            del h[k]
        h["logits_full"], h["dlogits_full"] = full, dfull
    return allr


def test_gathered_logits_path():
    allr, cfgs, hcs = T.emu_tp(_config(2), 2, 1, False)
    for res in _check_all(_as_gathered_logits(allr), cfgs, hcs):
        assert "logits gather" in res and "ce parts" not in res and "dlogits" in res
    Vs = allr[0]["head"]["logits"].shape[1]
    swapped = torch.cat([allr[0]["head"]["logits_full"][:, Vs:], allr[0]["head"]["logits_full"][:, :Vs]], 1)
    allr[1]["head"]["logits_full"] = swapped   # rank 1 gathers the shards in the wrong order
    _, fails = T.check_tp(allr, 1, cfgs[1], hcs[1], "emu", keep_going=True)
    assert fails and fails[0].startswith("stage logits gather: "), fails
    allr, cfgs, hcs = T.emu_tp(_config(2), 2, 1, False)
    _as_gathered_logits(allr)
    allr[0]["head"]["dlogits"] = allr[1]["head"]["dlogits"]   # rank 0 keeps rank 1's columns of the gradient
    _, fails = T.check_tp(allr, 0, cfgs[0], hcs[0], "emu", keep_going=True)
    assert any(f.startswith("stage dlogits: ") and "this rank's columns" in f for f in fails), fails


def test_missing_role_is_an_error():
    allr, cfgs, hcs = T.emu_tp(_config(2), 2, 1, True)
    del allr[0]["layers"][0]["ch"][0]["dW_o"]
    with pytest.raises(AssertionError, match="role 'dW_o': no recorded call produces it"):
        T.check_tp(allr, 0, cfgs[0], hcs[0], "emu")


def test_layout_is_the_documented_one():
    """W 2, c 2, T 8: chunk 0 is rows 0-3, chunk 1 rows 4-7; rank 0 holds rows 0, 1, 4, 5 and rank 1 rows 2, 3, 6, 7."""
    full = torch.arange(8.0)[:, None]
    s0, s1 = T.my_rows(full, 2, 0, 2), T.my_rows(full, 2, 1, 2)
    assert s0.reshape(-1).tolist() == [0, 1, 4, 5] and s1.reshape(-1).tolist() == [2, 3, 6, 7]
    assert T.layout([s0, s1], 2).reshape(-1).tolist() == list(range(8))


def test_sum_bounds():
    """W 2 by bits; W 4 under (W - 1) 2^-9 sum |a_i| (bf16) / 2^-24 (f32): one rounding of the exact sum passes, a
    value one bf16 ulp off a same-sign sum does not."""
    g = torch.Generator().manual_seed(0)
    p = [torch.rand(64, 64, generator=g).to(BF) + 1 for _ in range(4)]
    two = (p[0].float() + p[1].float()).to(BF)
    assert T.check_sum("s", two, p[:2], "emu") == 0.0
    with pytest.raises(AssertionError, match="differ by bits"):
        T.check_sum("s", torch.nextafter(two.float(), torch.tensor(9.0)).to(BF) + 2.0 ** -6, p[:2], "emu")
    four = sum(x.double() for x in p).float().to(BF)
    assert T.check_sum("s", four, p, "emu") <= 1.0
    T.check_sum("s", four + 2.0 ** -5, p, "emu")   # one ulp of [4, 8): 2^-5 > 3 * 2^-9 * 8
    assert T.OVER and "over the bound" in T.OVER[0]
    del T.OVER[:]
    f = [x.float() for x in p]
    assert T.check_sum("s", sum(x.double() for x in f).float(), f, "emu") <= 1.0


# ------------------------------------------------------------------------------ the ledger
@pytest.mark.parametrize("W,c", [(2, 1), (2, 2), (4, 2)])
def test_ledger_passes_production_order(W, c):
    for rank in range(W):
        assert T.check_waits(T.EmuTrace(W, rank, c).calls) == 2 * 2 * 2 * c   # gathers + scatters of 2 blocks, twice


@pytest.mark.parametrize("fault", [f for f in T.FAULTS if T.FAULT_ROLE[f][1] == "wait ledger"])
def test_ledger_rejects(fault):
    (W, c, _), _, word = T.FAULT_ROLE[fault]
    with pytest.raises(AssertionError, match="wait ledger") as e:
        T.check_waits(T.EmuTrace(W, 0, c, fault).calls)
    assert word in str(e.value), str(e.value)
    print(f"{fault}: {str(e.value)[:170]}")


def test_ledger_rejects_a_second_wait_and_a_write_to_an_input():
    tr = T.EmuTrace(2, 0, 2)
    first = next(c for c in tr.calls if c.name == "wait")
    tr.wait(first.of)
    with pytest.raises(AssertionError, match="second time"):
        T.check_waits(tr.calls)
    for drop_node_end, word in ((False, "returns with the handle"), (True, "is never waited")):
        tr = T.EmuTrace(2, 0, 1)   # a collective nobody reads or waits for: caught where the node returns, or at the end
        end = tr.calls.pop()
        tr.issue("all_reduce", torch.zeros(2, 2), torch.zeros(2, 2))
        tr.calls += [] if drop_node_end else [end]
        with pytest.raises(AssertionError, match=word):
            T.check_waits(tr.calls)
    tr = T.EmuTrace(2, 0, 1)
    i = next(i for i, c in enumerate(tr.calls) if c.name == "reduce_scatter_rows_into")
    src = tr.calls[i].ins[0].obj
    writer = M.Call("swiglu_bwd", (), {"dg": M.Rec(src, src)})   # a kernel writing the scatter's input while it is in flight
    writer.kwargs["dg"].post = src
    tr.calls.insert(i + 1, writer)
    with pytest.raises(AssertionError, match="the input of reduce_scatter_rows_into"):
        T.check_waits(tr.calls)


# ------------------------------------------------------------------------------ the recorder of the collectives
class _Work:
    def __init__(self, log):
        self.log = log

    def wait(self):
        self.log.append("real wait")


def test_recorder_logs_issue_and_wait_and_always_returns_a_handle(monkeypatch):
    from picotron_amd import functional as FN
    real_waits = []

    def all_gather(self, out, t, async_op=False):   # gloo's list form: done at the return, no handle
        out.copy_(torch.cat([t] * self.world_size))
        return None

    def all_reduce(self, t, async_op=False):
        t.mul_(self.world_size)
        return _Work(real_waits) if async_op else None
    monkeypatch.setattr(FN.TPContext, "all_gather_rows_into", all_gather)
    monkeypatch.setattr(FN.TPContext, "all_reduce", all_reduce)
    tp = FN.TPContext(group=None, world_size=2, rank=1)
    rec = M.Recorder(types_module())
    full, shard, mine, other = torch.zeros(8, 4), torch.ones(2, 4), torch.ones(2, 4), torch.ones(3)
    with T.recording_collectives(rec):
        h0 = tp.gather_chunk(full, shard, 1, 0, async_op=True)   # through all_gather_rows_into
        h1 = tp.all_reduce(mine, async_op=True)
        assert tp.all_reduce(other) is None                      # synchronous: complete at the return, nothing to wait for
        FN.wait_all([h0, h1])                                    # production's wait: neither handle is None
    assert FN.TPContext.all_reduce is all_reduce                 # restored
    assert [c.name for c in rec.calls] == ["all_gather_rows_into", "all_reduce", "all_reduce", "wait", "wait"]
    g, a, s, w0, w1 = rec.calls
    assert w0.of is g and w1.of is a and real_waits == ["real wait"] and (g.sync, a.sync, s.sync) == (False, False, True)
    assert g.outs[0].key == (full[:4].data_ptr(), (4, 4), (4, 1), F32) and g.ins[0].key[0] == shard.data_ptr()
    assert torch.equal(a.ins[0].pre, torch.ones(2, 4)) and torch.equal(a.outs[0].post, 2 * torch.ones(2, 4))
    assert torch.equal(g.outs[0].post, torch.ones(4, 4))
    assert T.check_waits(rec.calls) == 2


def types_module():
    import types
    return types.ModuleType("no_kernels")


# ------------------------------------------------------------------------------ the gloo sums of more than two ranks
def _wide_sum_rank(rank, world):
    import torch.distributed as dist
    from picotron_amd import functional as FN
    tp = FN.TPContext(dist.group.WORLD, world, rank)
    parts = [(torch.randn(16, 64, generator=torch.Generator().manual_seed(q)) + 1).to(BF) for q in range(world)]
    want = sum(p.double() for p in parts).float().to(BF)   # one rounding of the exact sum
    t = parts[rank].clone()
    assert tp.all_reduce(t, async_op=True) is None and t.dtype == BF   # complete at the return
    R.check_exact("all_reduce", t, want)
    out = torch.empty(16 // world, 64, dtype=BF)
    src = parts[rank].clone()
    assert tp.reduce_scatter_rows_into(out, src, async_op=True) is None
    R.check_exact("reduce_scatter_rows_into", out, want[rank * out.shape[0]:(rank + 1) * out.shape[0]])
    R.check_exact("reduce_scatter_rows_into leaves its input", src, parts[rank])
    f = parts[rank].float()
    tp.all_reduce(f)   # f32 partials: the transport's own sum
    assert f.dtype == F32 and T.check_sum("f32", f, [p.float() for p in parts], "emu") <= 1.0


def test_gloo_sums_more_than_two_bf16_partials_with_one_rounding():
    from tests import _dist
    _dist.run(_wide_sum_rank, 4)
