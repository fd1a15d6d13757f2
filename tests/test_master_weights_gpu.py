"""AdamW with fp32 master weights and moments (csrc/adamw.hip's adamw_master_* kernels,
optim.AdamW(master_weights=True, use_main_grad=True), DataParallelBucket.publish_grad): against
torch's f32 AdamW, the bit-for-bit equivalences between its forms, the global norm over mixed lists,
the non-finite skip, the state dict, and the dp2 / tp2 paths end to end."""
import math

import pytest
import torch

from tests import _dist

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32

# ragged tails, several tensors inside one workgroup's run, one tensor over many workgroups.
# The launch geometry at these sizes (csrc/adamw.hip, multi_grid): 131474 chunks of 8 elements,
# min(cap, ceil(chunks / 512)) = 257 workgroups of 256 threads (cap 1024 for the step, 2048 for the
# norm pass), each owning ceil(chunks / 257) = 512 chunks: two per thread, so the step's one-chunk-
# ahead pipeline runs both its prologue and its steady state; (512, 2048) spans 256 workgroups.
SHAPES = [(2048,), (1001,), (512, 2048), (37,), (3, 5, 7), (8,)]
CHUNKS = sum((math.prod(s) + 7) // 8 for s in SHAPES)
SC = dict(decay=1 - 3e-4 * 0.01, w1=0.1, beta2=0.999, c2=0.001, bc2_sqrt=(1 - 0.999 ** 3) ** 0.5, eps=1e-8,
          step_size=-3e-4 / (1 - 0.9 ** 3))


def _grads(seed=5, shapes=SHAPES, dtype=BF16):
    """seeded randn * 0.1, one tensor scaled by 1e2 and one by 1e-3"""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    out[1] *= 1e2
    out[3] *= 1e-3
    return [t.to(dtype).to(DEV) for t in out]


def _weights(seed=3, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(BF16).to(DEV) for s in shapes]


def _items(grads, seed=3):
    """[(master, param, grad, exp_avg, exp_avg_sq)] with non-zero moments"""
    g = torch.Generator().manual_seed(seed + 100)
    P = _weights(seed)
    out = []
    for p, gr in zip(P, grads):
        m = (torch.randn(p.shape, generator=g) * 0.01).to(DEV)
        v = (torch.randn(p.shape, generator=g).abs() * 1e-4).to(DEV)
        out.append((p.float(), p.clone(), gr.clone(), m, v))
    return out


def _sq64(tensors):
    return sum(t.detach().double().pow(2).sum().item() for t in tensors)


def _unaligned(n, seed, scale=1.0):
    """a bf16 view 2 bytes past a 16-byte boundary"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(n + 8, generator=g) * scale).to(BF16).to(DEV)
    v = base[1:1 + n]
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


def _eq_items(a, b, fields=(0, 1, 3, 4)):
    for x, y in zip(a, b):
        for f in fields:
            assert x[f].dtype == y[f].dtype and torch.equal(x[f], y[f]), f


def _state_of(opt, params):
    return [(opt.state[p]["master_param"], p.detach(), None, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            for p in params]


# ---------------------------------------------------------------- 1. against torch's f32 AdamW
@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["bf16_grad", "f32_grad"])
def test_against_torch_fp32_adamw(gdtype):
    from picotron_amd.optim import AdamW
    kw = dict(lr=3e-4, weight_decay=0.01)
    W = _weights()
    ours = [torch.nn.Parameter(w.clone()) for w in W]
    ref = [torch.nn.Parameter(w.float()) for w in W]
    oopt = AdamW(ours, master_weights=True, use_main_grad=True, **kw)
    ropt = torch.optim.AdamW(ref, foreach=True, **kw)
    for k in range(4):
        G = _grads(seed=50 + k, dtype=gdtype)
        for p, q, g in zip(ours, ref, G):
            p.main_grad = g          # bf16 or f32: p.grad could only hold bf16
            q.grad = g.float()
        oopt.step()
        ropt.step()
    torch.cuda.synchronize()
    for p, q in zip(ours, ref):
        so, sr = oopt.state[p], ropt.state[q]
        assert float(so["step"]) == float(sr["step"]) == 4.0
        assert p.dtype == BF16 and p.grad is None
        for a, b in ((so["master_param"], q.detach()), (so["exp_avg"], sr["exp_avg"]), (so["exp_avg_sq"], sr["exp_avg_sq"])):
            assert a.dtype == F32 and a.shape == b.shape
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (a - b).abs().max().item()
        assert torch.equal(p.detach(), so["master_param"].to(BF16))   # round to nearest even, exactly


# ------------------------------------------------------------------------- 2. equivalences
def test_list_launch_equals_per_tensor():
    from picotron_amd import kernels as K
    for gdtype in (BF16, F32):
        G = _grads(dtype=gdtype)
        a, b = _items(G), _items(G)
        K.adamw_master_step_multi(a, **SC)
        for it in b:
            K.adamw_master_step(*it, **SC)
        torch.cuda.synchronize()
        _eq_items(a, b)
        for it, it0 in zip(a, _items(G)):
            assert not torch.equal(it[0], it0[0]) and torch.equal(it[2], it0[2])
        # clipped, and the unaligned single-tensor form against the aligned one
        sq = K.grad_sqnorm(items=a)
        M = 0.25 * math.sqrt(_sq64(G))
        K.adamw_master_step_multi_clip(a, sq, M, **SC)
        for it in b:
            K.adamw_master_step_clip(*it, sq, M, **SC)
        torch.cuda.synchronize()
        _eq_items(a, b)
    n = 1001
    pu, gu = _unaligned(n, 1), _unaligned(n, 2, 0.1)
    w, m, v = pu.float(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pa, ga = pu.clone(), gu.clone()
    w2, m2, v2 = w.clone(), m.clone(), v.clone()
    K.adamw_master_step(w, pu, gu, m, v, **SC)
    K.adamw_master_step(w2, pa, ga, m2, v2, **SC)
    torch.cuda.synchronize()
    assert torch.equal(w, w2) and torch.equal(pu, pa) and torch.equal(m, m2) and torch.equal(v, v2)


@pytest.mark.parametrize("factor", [None, 0.25, 4.0], ids=["unclipped", "clip0.25", "clip4"])
def test_bf16_grads_equal_their_f32_copies(factor):
    """float(bf16 g) and the f32 copy of g are the same f32 number, and everything after the load is
    one expression: the two instantiations give the same bits (the norm passes too)."""
    from picotron_amd import kernels as K
    G = _grads()
    a, b = _items(G), _items([g.float() for g in G])
    if factor is None:
        K.adamw_master_step_multi(a, **SC)
        K.adamw_master_step_multi(b, **SC)
    else:
        M = factor * math.sqrt(_sq64(G))
        sa, sb = K.grad_sqnorm(items=a), K.grad_sqnorm(items=b)
        assert torch.equal(sa, sb)
        K.adamw_master_step_multi_clip(a, sa, M, **SC)
        K.adamw_master_step_multi_clip(b, sb, M, **SC)
    torch.cuda.synchronize()
    _eq_items(a, b)
    assert K.device_status(torch.device(DEV)) == 0


@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_fused_clip_equals_inplace_f32_scale(factor):
    """The clipped master step on f32 gradients == clip_grad_norm_'s in-place f32 scale (grad_scale),
    then the unclipped master step; the fused path leaves the gradients alone.  factor 4: both equal
    the unclipped step and the scale stores nothing."""
    from picotron_amd import kernels as K
    G = _grads(dtype=F32)
    norm = math.sqrt(_sq64(G))
    M = factor * norm
    a, b = _items(G), _items(G)
    sq = K.grad_sqnorm(items=a)
    K.adamw_master_step_multi_clip(a, sq, M, **SC)
    for it in b:
        K.grad_scale(it[2], sq, M)
    K.adamw_master_step_multi(b, **SC)
    torch.cuda.synchronize()
    _eq_items(a, b)
    for it, g in zip(a, G):
        assert torch.equal(it[2], g)   # bit-unchanged
    if factor < 1:
        coef = factor * norm / (norm + 1e-6)
        for it, g in zip(b, G):
            assert not torch.equal(it[2], g) and torch.allclose(it[2], g * coef, rtol=1e-5, atol=0)
    else:
        c = _items(G)
        K.adamw_master_step_multi(c, **SC)
        torch.cuda.synchronize()
        _eq_items(a, c)
        for it, g in zip(b, G):
            assert torch.equal(it[2], g)
    assert K.device_status(torch.device(DEV)) == 0


def test_two_runs_bit_equal():
    from picotron_amd.optim import AdamW
    runs = []
    for _ in range(2):
        params = [torch.nn.Parameter(w) for w in _weights()]
        opt = AdamW(params, lr=3e-4, master_weights=True, max_grad_norm=1.0)
        for k in range(2):
            for p, g in zip(params, _grads(seed=70 + k)):
                p.grad = g
            opt.step()
        torch.cuda.synchronize()
        runs.append((_state_of(opt, params), opt.last_grad_norm))
    _eq_items(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------- 3. norm
def test_f32_list_norm_against_fp64():
    from picotron_amd import kernels as K
    G = _grads(dtype=F32)
    sq64 = _sq64(G)
    blocks = min(2048, -(-CHUNKS // 512))
    per_block = -(-CHUNKS // blocks)
    assert blocks == 257 and per_block == 512
    # grad_sq_list_kernel, the one walk of the bf16 list's norm pass too: every term g * g >= 0 enters through
    # one fused multiply-add (the f32 square is not rounded on its own), so the relative error is at
    # most (f32 additions on the longest path from a term to the result) * 2^-24:
    #   in a thread: an accumulator takes 8 fused adds per chunk, from at most ceil(per_block / 256)
    #     chunks of one tensor plus one more per further tensor in the run, and up to 7 ragged
    #     elements per tensor;
    #   4 accumulators -> 1: 2; wave butterfly: 6; 4 waves: 3;
    #   final kernel: ceil(blocks / 256) per thread, 6, 3; the weight product: 1;  + 2 spare.
    nt = len(G)
    chain = 8 * (-(-per_block // 256) + nt) + 7 * nt
    adds = chain + 2 + 6 + 3 + -(-blocks // 256) + 6 + 3 + 1 + 2
    tol = adds * 2.0 ** -24
    assert tol <= 1e-5, tol
    items = _items(G)
    sq = K.grad_sqnorm(items=items)
    again = K.grad_sqnorm(items=items)
    torch.cuda.synchronize()
    print(f"sq {sq.item():.9e} fp64 {sq64:.9e} rel {abs(sq.item() - sq64) / sq64:.3e} tol {tol:.3e}")
    assert sq.dtype == F32 and sq.shape == (1,)
    assert abs(sq.double().item() - sq64) <= tol * sq64
    assert torch.equal(sq, again)
    half = K.grad_sqnorm(items=items, weight=0.5)
    assert half.item() == 0.5 * sq.item()
    for it, g in zip(items, G):
        assert torch.equal(it[2], g)


def test_mixed_optimizer_one_norm_one_coefficient():
    """A bf16-grad list, an f32-grad list (main_grad), an unaligned bf16 parameter and an f32
    parameter, in two param groups: one global norm (against fp64), one coefficient -- after step 1
    from zero moments exp_avg = 0.1 * coef * g, never through bf16."""
    from picotron_amd import optim
    G16 = _grads()[:3]
    G32 = _grads(seed=6, dtype=F32)[1:5]
    g = torch.Generator().manual_seed(8)
    gf = (torch.randn(3000, generator=g) * 0.3).to(DEV)
    gu = _unaligned(777, 12, 0.2)
    p16 = [torch.nn.Parameter(torch.zeros_like(t)) for t in G16]
    p32 = [torch.nn.Parameter(torch.zeros(t.shape, dtype=BF16, device=DEV)) for t in G32]
    pf = torch.nn.Parameter(torch.zeros_like(gf))
    pu = torch.nn.Parameter(_unaligned(777, 13))
    for p, t in zip(p16 + [pf, pu], G16 + [gf, gu]):
        p.grad = t
    for p, t in zip(p32, G32):
        p.main_grad = t
    params, grads = p16 + p32 + [pf, pu], G16 + G32 + [gf, gu]
    norm = math.sqrt(_sq64(grads))
    opt = optim.AdamW([dict(params=p16 + p32[:2]), dict(params=p32[2:] + [pf, pu], weight_decay=0.0)], lr=1e-3,
                      max_grad_norm=0.25 * norm, master_weights=True, use_main_grad=True)
    opt.step()
    torch.cuda.synchronize()
    got = opt.last_grad_norm.item()
    print(f"mixed norm {got:.9e} fp64 {norm:.9e} rel {abs(got - norm) / norm:.3e}")
    assert abs(got - norm) <= 1e-5 * norm, (got, norm)
    coef = torch.tensor(0.25 * norm / (norm + 1e-6), dtype=F32, device=DEV)
    for p, gr in zip(params, grads):
        st = opt.state[p]
        assert st["exp_avg"].dtype == F32 and ("master_param" in st) == (p.dtype == BF16)
        want = (gr.float() * coef) * 0.1
        assert torch.allclose(st["exp_avg"], want, rtol=1e-5, atol=1e-30), (p.shape, (st["exp_avg"] - want).abs().max().item())
        if p.dtype == BF16:
            assert torch.equal(p.detach(), st["master_param"].to(BF16))


# ------------------------------------------------------------------------ 4. non-finite skip
def test_nonfinite_norm_skips_the_master_step():
    from picotron_amd import _C
    from picotron_amd import kernels as K
    from picotron_amd.optim import AdamW
    K.device_status(torch.device(DEV))   # start from a clear word
    G = _grads()
    params = [torch.nn.Parameter(w) for w in _weights()] + [torch.nn.Parameter(_unaligned(777, 13))]
    opt = AdamW(params, lr=1e-3, max_grad_norm=1.0, master_weights=True)
    for p, gr in zip(params, G + [_unaligned(777, 12, 0.2)]):
        p.grad = gr.clone()
    opt.step()   # a first finite step: masters and moments exist and are not zero
    torch.cuda.synchronize()
    assert K.device_status(torch.device(DEV)) == 0

    def snap():
        return [tuple(None if t is None else t.clone() for t in it) for it in _state_of(opt, params)]
    before = snap()
    params[2].grad.view(-1)[12345] = float("inf")
    opt.step()
    torch.cuda.synchronize()
    _eq_items(_state_of(opt, params), before)
    assert not math.isfinite(opt.last_grad_norm.item())
    with pytest.raises(_C.HipKernelError, match="gradient norm"):
        K.check_device_status(torch.device(DEV))
    params[2].grad.view(-1)[12345] = 0.0
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(opt.last_grad_norm.item())
    for now, old in zip(_state_of(opt, params), before):
        for f in (0, 3, 4):   # (the bf16 weights of a small tensor may all stay: lr against their ulp)
            assert not torch.equal(now[f], old[f])
    assert not torch.equal(params[2].detach(), before[2][1])
    assert K.device_status(torch.device(DEV)) == 0
    K.check_device_status(torch.device(DEV))


# ------------------------------------------------------------- 5. what the feature is for
def test_small_updates_survive():
    """lr 3e-5 on N(0, 0.02) weights: most updates are below half a bf16 ulp of the weight.
    (i) master weights must move like (ii) torch's f32 AdamW published as bf16; (iii) today's bf16
    recipe, printed only (measured: ratio 0.30, 69 % of the elements unmoved)."""
    from picotron_amd.optim import AdamW
    gen = torch.Generator().manual_seed(0)
    p0 = (torch.randn(4096, generator=gen) * 0.02).to(BF16).to(DEV)
    grad = (torch.randn(4096, generator=gen) * 1e-3).to(BF16).to(DEV)
    kw = dict(lr=3e-5, weight_decay=0.0)
    pm, pr, pb = (torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.float()), torch.nn.Parameter(p0.clone()))
    om, orf, ob = AdamW([pm], master_weights=True, **kw), torch.optim.AdamW([pr], foreach=True, **kw), AdamW([pb], **kw)
    pm.grad, pr.grad, pb.grad = grad, grad.float(), grad
    for _ in range(50):
        om.step()
        orf.step()
        ob.step()
    torch.cuda.synchronize()
    ref = (pr.detach() - p0.float()).abs().mean().item()
    fig = {}
    for name, p in (("master", pm), ("bf16", pb)):
        d = p.detach().float() - p0.float()
        fig[name] = (d.abs().mean().item() / ref, (d == 0).float().mean().item())
        print(f"{name}: mean|dp| / f32's {fig[name][0]:.3f}, unmoved {100 * fig[name][1]:.1f} %")
    assert 0.97 <= fig["master"][0] <= 1.03, fig
    assert fig["master"][1] <= 0.01, fig


# ------------------------------------------------------------------------------ 6. state dict
def _stepped(master, steps=2, max_grad_norm=None):
    from picotron_amd.optim import AdamW
    params = [torch.nn.Parameter(w) for w in _weights()]
    opt = AdamW(params, lr=3e-4, master_weights=master, max_grad_norm=max_grad_norm)
    for k in range(steps):
        for p, g in zip(params, _grads(seed=80 + k)):
            p.grad = g
        opt.step()
    return params, opt


def test_state_dict_round_trip():
    from picotron_amd.optim import AdamW
    params, opt = _stepped(True)
    torch.cuda.synchronize()
    sd = opt.state_dict()
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = AdamW(fresh, lr=3e-4, master_weights=True)
    opt2.load_state_dict(sd)
    for p, q in zip(params, fresh):
        for k in ("master_param", "exp_avg", "exp_avg_sq"):
            a, b = opt.state[p][k], opt2.state[q][k]
            assert b.dtype == F32 and torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k
        assert float(opt2.state[q]["step"]) == 2.0 and opt2.state[q]["step"].dtype == F32
    for p, q, g in zip(params, fresh, _grads(seed=90)):
        p.grad, q.grad = g, g.clone()
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    _eq_items(_state_of(opt, params), _state_of(opt2, fresh))


def test_state_dict_across_modes():
    from picotron_amd.optim import AdamW
    params, plain = _stepped(False)
    torch.cuda.synchronize()
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = AdamW(fresh, lr=3e-4, master_weights=True)
    opt.load_state_dict(plain.state_dict())
    for p, q in zip(params, fresh):
        for k in ("exp_avg", "exp_avg_sq"):
            assert plain.state[p][k].dtype == BF16 and opt.state[q][k].dtype == F32
            assert torch.equal(opt.state[q][k], plain.state[p][k].float())
        assert "master_param" not in opt.state[q]
    for q, g in zip(fresh, _grads(seed=90)):
        q.grad = g
    before = [q.detach().clone() for q in fresh]
    opt.step()
    torch.cuda.synchronize()
    for q, b in zip(fresh, before):
        st = opt.state[q]
        assert float(st["step"]) == 3.0 and st["master_param"].dtype == F32
        # the master moved off the weight it was read from (a small tensor's bf16 weights need not:
        # lr is below half their ulp)
        assert torch.equal(q.detach(), st["master_param"].to(BF16)) and not torch.equal(st["master_param"], b.float())
    # the other direction: f32 state into the bf16 recipe
    other = AdamW([torch.nn.Parameter(p.detach().clone()) for p in params], lr=3e-4)
    with pytest.raises(ValueError, match="master_weights"):
        other.load_state_dict(opt.state_dict())


def test_sync_master_from_params():
    params, opt = _stepped(True, steps=1)
    with torch.no_grad():
        for p in params:
            p.mul_(2.0)
    opt.sync_master_from_params()
    torch.cuda.synchronize()
    for p in params:
        assert torch.equal(opt.state[p]["master_param"], p.detach().float())


# --------------------------------------------------------------------------- 7. use_main_grad
def test_use_main_grad():
    from picotron_amd.optim import AdamW
    G = _grads(dtype=F32)
    a = [torch.nn.Parameter(w) for w in _weights()]
    b = [torch.nn.Parameter(w) for w in _weights()]
    for p, g in zip(a, G):
        p.main_grad, p.grad = g.clone(), None
    oa = AdamW(a, lr=3e-4, master_weights=True, use_main_grad=True)
    oa.step()
    # The same step fed those tensors as the gradient: torch refuses an f32 p.grad on a bf16
    # parameter, so they go to the list launch directly, on the state step 1 starts from and with
    # step 1's scalars (optim.AdamW._batches' expressions).
    from picotron_amd import kernels as K
    with pytest.raises(RuntimeError):
        b[0].grad = G[0]
    items = [(q.detach().float(), q.detach().clone(), g, torch.zeros(q.shape, device=DEV), torch.zeros(q.shape, device=DEV))
             for q, g in zip(b, G)]
    lr, wd, beta1, beta2 = 3e-4, 1e-2, 0.9, 0.999
    K.adamw_master_step_multi(items, decay=1 - lr * wd, w1=1 - beta1, beta2=beta2, c2=1 - beta2,
                              bc2_sqrt=(1 - beta2 ** 1.0) ** 0.5, eps=1e-8, step_size=(lr / (1 - beta1 ** 1.0)) * -1)
    torch.cuda.synchronize()
    _eq_items(_state_of(oa, a), items)
    assert all(p.grad is None for p in a) and all(torch.equal(p.main_grad, g) for p, g in zip(a, G))
    # a parameter without main_grad falls back to p.grad; one with both uses main_grad
    g16 = _grads()
    c = [torch.nn.Parameter(w) for w in _weights()]
    d = [torch.nn.Parameter(w) for w in _weights()]
    for i, (p, q) in enumerate(zip(c, d)):
        p.grad = g16[i].clone()
        q.grad = g16[i].clone() if i % 2 else torch.full_like(g16[i], 7.0)
        if i % 2 == 0:
            q.main_grad = g16[i].clone()
    oc = AdamW(c, lr=3e-4, master_weights=True)
    od = AdamW(d, lr=3e-4, master_weights=True, use_main_grad=True)
    oc.step()
    od.step()
    torch.cuda.synchronize()
    _eq_items(_state_of(oc, c), _state_of(od, d))
    with pytest.raises(ValueError, match="master_weights"):
        AdamW(c, use_main_grad=True)


def test_non_contiguous_parameter_goes_per_tensor():
    """A transposed view (non-contiguous weights and gradient) takes the single-tensor path through a
    dense copy: the same bits as its contiguous twin in the list launch; a skipped step leaves it alone."""
    from picotron_amd import kernels as K
    from picotron_amd.optim import AdamW
    K.device_status(torch.device(DEV))
    g = torch.Generator().manual_seed(4)
    w = torch.randn(48, 64, generator=g).to(BF16).to(DEV)
    gr = (torch.randn(48, 64, generator=g) * 0.1).to(BF16).to(DEV)
    a, b = torch.nn.Parameter(w.clone().t()), torch.nn.Parameter(w.t().contiguous())
    assert not a.is_contiguous() and b.is_contiguous()
    oa = AdamW([a], lr=1e-2, master_weights=True)
    ob = AdamW([b], lr=1e-2, master_weights=True)
    for _ in range(2):
        a.grad, b.grad = gr.clone().t(), gr.t().contiguous()
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert not a.is_contiguous() and not torch.equal(a.detach(), w.t())
    _eq_items(_state_of(oa, [a]), _state_of(ob, [b]))
    # clipped (the norm of a single tensor has its own add chain: no bit comparison with the list)
    oc = AdamW([a], lr=1e-2, master_weights=True, max_grad_norm=1.0)
    oc.step()
    torch.cuda.synchronize()
    want = math.sqrt(_sq64([gr]))
    assert abs(oc.last_grad_norm.item() - want) <= 1e-5 * want
    keep = a.detach().clone()
    assert not torch.equal(keep, b.detach())
    a.grad[3, 5] = float("nan")
    oc.step()
    torch.cuda.synchronize()
    assert torch.equal(a.detach(), keep)
    assert K.device_status(torch.device(DEV)) == K.STATUS_NONFINITE_GRAD


# ------------------------------------------------------------------------------- multi-rank
def _dp2_body(rank, world):
    import types
    import os
    import torch.distributed as dist
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    from oracle import picotron_oracle as O
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import train
    from picotron_amd.context_parallel.context_parallel import apply_context_parallel
    from picotron_amd.data_parallel.data_parallel import DataParallelBucket
    from picotron_amd.model import Llama
    from picotron_amd.optim import AdamW
    from tests.test_parallel_gpu import CFG
    pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=world)
    full = {k: v.to(BF16) for k, v in O.init_params(dict(CFG), seed=9).items()}
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**CFG))
    apply_context_parallel(model)
    model.to(BF16)
    names = dict(model.named_parameters())
    with torch.no_grad():
        for n, p in names.items():
            p.copy_(full[n])
    ddp = DataParallelBucket(model)
    assert ddp.publish_grad is True
    ddp.publish_grad = False
    loader = train.SyntheticMicroBatchDataLoader(2, CFG["max_position_embeddings"], 2, CFG["vocab_size"], "cuda")
    train.train_step(ddp, loader, torch.device("cuda"))
    torch.cuda.synchronize()
    assert all(p.grad is None for p in names.values())
    assert all(p.main_grad.dtype == F32 for p in names.values())
    norm64 = math.sqrt(_sq64([p.main_grad for p in names.values()]))
    M = 0.25 * norm64
    mg = {n: p.main_grad.clone() for n, p in names.items()}
    opt = AdamW(model.parameters(), lr=1e-3, master_weights=True, use_main_grad=True, max_grad_norm=M)
    opt.step()
    torch.cuda.synchronize()
    got = opt.last_grad_norm.item()
    assert abs(got - norm64) <= 1e-5 * norm64, (got, norm64)
    coef = torch.tensor(M / (got + 1e-6), dtype=F32, device="cuda")
    for n, p in names.items():
        st = opt.state[p]
        assert p.grad is None and torch.equal(p.main_grad, mg[n])
        want = (mg[n] * coef) * 0.1
        assert torch.allclose(st["exp_avg"], want.view_as(st["exp_avg"]), rtol=1e-5, atol=1e-30), n
        assert torch.equal(p.detach(), st["master_param"].to(BF16)), n
        assert not torch.equal(st["master_param"], full[n].cuda().float()), n   # (lr < half a bf16 ulp of a norm weight)
    # both ranks hold the same bits: weights, masters, the norm
    flat = torch.cat([torch.cat([p.detach().float().view(-1), opt.state[p]["master_param"].view(-1)])
                      for p in names.values()] + [opt.last_grad_norm.view(1)]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert torch.equal(both[0], both[1])


def test_dp2_main_grad_end_to_end():
    _dist.run(_dp2_body, 2, device="cuda")


def _tp2_body(rank, world):
    import torch.distributed as dist
    from picotron_amd import functional as FN
    from picotron_amd.optim import AdamW
    from tests.test_parallel_gpu import CFG, TOL, _setup
    m, model, names, pf, ids, lo, loss_r = _setup(2, 1)
    V = CFG["vocab_size"]
    logits = model(ids[:, :-1].cuda())
    FN.cross_entropy(logits.view(-1, V), ids[:, 1:].reshape(-1).cuda()).backward()
    oracle_norm = math.sqrt(sum(pf[n].grad.double().pow(2).sum().item() for n in names))
    opt = AdamW(model.parameters(), max_grad_norm=0.25 * oracle_norm, master_weights=True)
    opt.step()
    torch.cuda.synchronize()
    got = opt.last_grad_norm.item()
    assert abs(got - oracle_norm) < TOL * oracle_norm, (got, oracle_norm)
    rep = [n for n, p in names.items() if not getattr(p, "tensor_model_parallel", False)]
    assert 0 < len(rep) < len(names)
    flat = torch.cat([torch.cat([names[n].detach().float().view(-1), opt.state[names[n]]["master_param"].view(-1)])
                      for n in rep] + [opt.last_grad_norm.view(1)]).cpu()
    both = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert torch.equal(both[0], both[1])
    for n, p in names.items():
        assert torch.equal(p.detach(), opt.state[p]["master_param"].to(BF16)), n


def test_tp2_llama_clipped_master_step():
    _dist.run(_tp2_body, 2, device="cuda")
