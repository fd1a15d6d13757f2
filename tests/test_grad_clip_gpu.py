"""Global gradient-norm clipping fused into the AdamW step (csrc/adamw.hip, optim.AdamW(max_grad_norm=),
optim.clip_grad_norm_): the f32 norm pass against float64, the fused scale against the in-place
scale bit for bit, the optimizer against torch's clip_grad_norm_ + AdamW, the non-finite skip, and
the reduction of the norm over tensor- and pipeline-parallel ranks."""
import math

import pytest
import torch

from tests import _dist

DEV = "cuda"
pytestmark = pytest.mark.gpu

# ragged tails, several tensors inside one workgroup's run, 257 workgroups over the large tensor
SHAPES = [(2048,), (1001,), (512, 2048), (37,), (3, 5, 7), (8,)]
SC = dict(decay=1 - 3e-4 * 0.01, w1=0.1, beta2=0.999, c2=0.001, bc2_sqrt=(1 - 0.999 ** 3) ** 0.5, eps=1e-8,
          step_size=-3e-4 / (1 - 0.9 ** 3))


def _grads(seed=5, shapes=SHAPES, dtype=torch.bfloat16):
    """seeded randn * 0.1, one tensor scaled by 1e2 and one by 1e-3"""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    out[1] *= 1e2
    out[3] *= 1e-3
    return [t.to(dtype).to(DEV) for t in out]


def _state(seed=3, shapes=SHAPES, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)

    def mk():
        return [torch.randn(s, generator=g).to(dtype).to(DEV) for s in shapes]
    return mk(), [t.abs() * 0.01 for t in mk()], [t.abs() * 1e-4 for t in mk()]


def _sq64(tensors):
    return sum(t.detach().double().pow(2).sum().item() for t in tensors)


def _only(grads):
    return [(g, g, g, g) for g in grads]


def _unaligned(n, seed, scale=1.0):
    """a bf16 view 2 bytes past a 16-byte boundary"""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(n + 8, generator=g) * scale).to(torch.bfloat16).to(DEV)
    v = base[1:1 + n]
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


def test_sqnorm_against_fp64():
    from picotron_amd import kernels as K
    G = _grads()
    sq64 = _sq64(G)
    # The launch geometry at these sizes (csrc/adamw.hip, pt_grad_sq_multi): chunks of 8 elements,
    # min(2048, ceil(chunks / 512)) workgroups of 256 threads, each owning ceil(chunks / workgroups).
    chunks = sum((t.numel() + 7) // 8 for t in G)
    blocks = min(2048, -(-chunks // 512))
    per_block = -(-chunks // blocks)
    assert blocks == 257 and per_block == 512
    # Every term is >= 0 (and a bf16 square is exact in f32), so the relative error is at most
    # (number of f32 additions on the longest path from a term to the result) * 2^-24:
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
    sq = K.grad_sqnorm(items=_only(G))
    again = K.grad_sqnorm(items=_only(G))
    torch.cuda.synchronize()
    print(f"sq {sq.item():.9e} fp64 {sq64:.9e} rel {abs(sq.item() - sq64) / sq64:.3e} tol {tol:.3e}")
    assert sq.dtype == torch.float32 and sq.shape == (1,)
    assert abs(sq.double().item() - sq64) <= tol * sq64
    assert torch.equal(sq, again)
    # the single-tensor form (f32, unaligned bf16) under the same bound, its own geometry:
    # min(2048, ceil(n / 256)) workgroups, grid-strided, 4 accumulators
    for t in (_grads(dtype=torch.float32)[2], _unaligned(100003, 9, 0.1)):
        n = t.numel()
        wg = min(2048, -(-n // 256))
        per_thread = -(-n // (wg * 256))
        adds1 = -(-per_thread // 4) + 1 + 2 + 6 + 3 + -(-wg // 256) + 6 + 3 + 1 + 2
        # f32 inputs: the square itself is rounded (fused into the add, so it costs nothing extra)
        one = K.grad_sqnorm(tensors=[t])
        two = K.grad_sqnorm(tensors=[t])
        ref = _sq64([t])
        assert abs(one.double().item() - ref) <= adds1 * 2.0 ** -24 * ref, (one.item(), ref)
        assert torch.equal(one, two)
    # accumulation in stream order and the list's weight
    acc = K.grad_sqnorm(items=_only(G[:3]))
    K.grad_sqnorm(items=_only(G[3:]), out=acc, accumulate=True)
    assert abs(acc.double().item() - sq64) <= 2 * tol * sq64
    half = K.grad_sqnorm(items=_only(G), weight=0.5)
    assert half.item() == 0.5 * sq.item()
    zero = K.grad_sqnorm(items=_only([torch.zeros_like(t) for t in G]))
    assert zero.item() == 0.0


def _eq_lists(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_fused_equals_unfused_multi(factor):
    """adamw_step_multi_clip on the original gradients == the in-place scale, then today's
    adamw_step_multi, bit for bit; the fused path leaves the gradients alone.  factor 4: clipping is
    inactive and both equal the unclipped step, the scale stores nothing."""
    from picotron_amd import kernels as K
    G = _grads()
    P, M, V = _state()
    norm = math.sqrt(_sq64(G))
    max_norm = factor * norm
    a = [[t.clone() for t in L] for L in (P, G, M, V)]
    b = [[t.clone() for t in L] for L in (P, G, M, V)]
    sq = K.grad_sqnorm(items=list(zip(*a)))
    K.adamw_step_multi_clip(list(zip(*a)), sq, max_norm, **SC)
    K.grad_scale_multi(list(zip(*b)), sq, max_norm)
    K.adamw_step_multi(list(zip(*b)), **SC)
    torch.cuda.synchronize()
    for i in (0, 2, 3):
        _eq_lists(a[i], b[i])
    _eq_lists(a[1], G)   # path A's gradients are bit-unchanged
    if factor < 1:
        assert all(not torch.equal(x, y) for x, y in zip(b[1], G))   # path B's were scaled
        coef = factor * norm / (norm + 1e-6)
        for x, y in zip(b[1], G):   # ... by about the coefficient (bf16 rounding)
            assert torch.allclose(x.float(), y.float() * coef, rtol=2 ** -7, atol=0)
    else:
        _eq_lists(b[1], G)
        c = [[t.clone() for t in L] for L in (P, G, M, V)]
        K.adamw_step_multi(list(zip(*c)), **SC)
        torch.cuda.synchronize()
        for i in (0, 2, 3):
            _eq_lists(a[i], c[i])
    assert K.device_status(torch.device(DEV)) == 0


@pytest.mark.parametrize("kind", ["f32", "bf16_unaligned"])
@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_fused_equals_unfused_single(kind, factor):
    from picotron_amd import kernels as K
    n = 1001
    if kind == "f32":
        g = torch.Generator().manual_seed(21)
        P, G, M, V = (torch.randn(n, generator=g).to(DEV), (torch.randn(n, generator=g) * 0.1).to(DEV),
                      (torch.randn(n, generator=g).abs() * 0.01).to(DEV),
                      (torch.randn(n, generator=g).abs() * 1e-4).to(DEV))
    else:
        P, G, M, V = _unaligned(n, 1), _unaligned(n, 2, 0.1), _unaligned(n, 3, 0.01), _unaligned(n, 4, 1e-2)
        M.abs_()   # in place: the views stay unaligned
        V.abs_()
    norm = math.sqrt(_sq64([G]))
    max_norm = factor * norm

    def copies():
        if kind == "f32":
            return [t.clone() for t in (P, G, M, V)]
        out = []
        for t in (P, G, M, V):
            base = torch.empty(n + 8, dtype=t.dtype, device=DEV)
            v = base[1:1 + n]
            v.copy_(t)
            out.append(v)
        return out
    a, b = copies(), copies()
    sq = K.grad_sqnorm(tensors=[a[1]])
    K.adamw_step_clip(*a, sq, max_norm, **SC)
    K.grad_scale(b[1], sq, max_norm)
    K.adamw_step(*b, **SC)
    torch.cuda.synchronize()
    for i in (0, 2, 3):
        assert torch.equal(a[i], b[i])
        assert not torch.equal(a[i], (P, G, M, V)[i])
    assert torch.equal(a[1], G)
    if factor < 1:
        assert not torch.equal(b[1], G)
    else:
        assert torch.equal(b[1], G)
        c = copies()
        K.adamw_step(*c, **SC)
        torch.cuda.synchronize()
        for i in (0, 2, 3):
            assert torch.equal(a[i], c[i])


def test_scale_against_torch():
    """grad = bf16(g * coef): torch's expression on the kernel's own sq; a coefficient one or two f32
    ulps away moves about 2^-15 of the elements across a bf16 rounding boundary, by one ulp."""
    from picotron_amd import kernels as K
    G = _grads()
    out = [t.clone() for t in G]
    norm = math.sqrt(_sq64(G))
    max_norm = 0.25 * norm
    sq = K.grad_sqnorm(items=_only(out))
    K.grad_scale_multi(_only(out), sq, max_norm)
    coef_t = (max_norm / (sq.sqrt() + 1e-6)).clamp(max=1.0)
    assert coef_t.dtype == torch.float32 and 0.2 < coef_t.item() < 0.3
    differ = total = 0
    for o, g in zip(out, G):
        want = (g.float() * coef_t).to(torch.bfloat16)
        oi, wi = o.view(torch.int16).int(), want.view(torch.int16).int()
        assert ((oi - wi).abs() <= 1).all()           # equal or one bf16 ulp apart (same sign: ordered bits)
        differ += (oi != wi).sum().item()
        total += o.numel()
    print(f"scale vs torch: {differ} of {total} elements differ")
    assert differ <= 1e-3 * total


def _clip_run(steps, shapes, dtype, max_norm, seed=0):
    """(ours, reference): optim.AdamW(max_grad_norm) against clip_grad_norm_ on f32 copies of the
    gradients, cast back, then torch.optim.AdamW(foreach=True); different seeded gradients per step."""
    from picotron_amd.optim import AdamW
    kw = dict(lr=3e-4, weight_decay=0.01)
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=g).to(dtype).to(DEV) for s in shapes]
    scales = [1.0, 8.0, 0.5, 6.0][:steps]
    grads = [[(torch.randn(s, generator=g) * 0.1 * sc).to(dtype).to(DEV) for s in shapes] for sc in scales]
    ours = [torch.nn.Parameter(t.clone()) for t in init]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    oopt = AdamW(ours, max_grad_norm=max_norm, **kw)
    ropt = torch.optim.AdamW(ref, foreach=True, **kw)
    norms_o, norms_r = [], []
    for k in range(steps):
        for p, gr in zip(ours, grads[k]):
            p.grad = gr.clone()
        oopt.step()
        norms_o.append(oopt.last_grad_norm)
        f32 = [torch.nn.Parameter(gr.float()) for gr in grads[k]]
        for q, gr in zip(f32, grads[k]):
            q.grad = gr.float()
        norms_r.append(torch.nn.utils.clip_grad_norm_(f32, max_norm))
        for p, q in zip(ref, f32):
            p.grad = q.grad.to(dtype)
        ropt.step()
        for p, gr in zip(ours, grads[k]):
            assert torch.equal(p.grad, gr)   # the fused clip never writes the gradients
    torch.cuda.synchronize()
    return (ours, oopt, norms_o), (ref, ropt, norms_r)


def test_optimizer_against_torch():
    shapes = [(2048,), (1001,), (512, 2048), (37,), (3, 5, 7), (8,)]
    n = sum(math.prod(s) for s in shapes)
    M = 2.0 * 0.1 * math.sqrt(n)   # between the steps' norms: about 0.1 sqrt(n) * (1, 8, 0.5, 6)
    (ours, oopt, norms_o), (ref, ropt, norms_r) = _clip_run(4, shapes, torch.bfloat16, M)
    nr = [x.item() for x in norms_r]
    assert sum(x > M for x in nr) >= 2 and sum(x < M for x in nr) >= 1, (nr, M)
    for a, b in zip(norms_o, norms_r):
        assert a.dtype == torch.float32 and a.dim() == 0 and a.is_cuda
        assert abs(a.item() - b.item()) <= 1e-5 * b.item(), (a.item(), b.item())
    for pr, po in zip(ref, ours):
        sr, so = ropt.state[pr], oopt.state[po]
        assert float(sr["step"]) == float(so["step"]) == 4.0
        for a, b in ((pr, po), (sr["exp_avg"], so["exp_avg"]), (sr["exp_avg_sq"], so["exp_avg_sq"])):
            a, b = a.detach().float().cpu(), b.detach().float().cpu()
            diff = (a != b)
            assert diff.float().mean().item() < 1e-3, diff.float().mean().item()
            assert ((a - b).abs() <= 1e-2 * a.abs().clamp_min(1e-3)).all()


def test_mixed_list_one_coefficient():
    """bf16 list + an f32 tensor + an unaligned bf16 view in one optimizer: one global norm over all
    of them (against fp64), and every tensor scaled by the same coefficient -- after step 1 from
    zero moments exp_avg = 0.1 * coef * g."""
    from picotron_amd.optim import AdamW
    G = _grads()[:4]
    g = torch.Generator().manual_seed(8)
    gf = (torch.randn(3000, generator=g) * 0.3).to(DEV)
    gu = _unaligned(777, 12, 0.2)
    pu = torch.nn.Parameter(_unaligned(777, 13))
    params = [torch.nn.Parameter(torch.zeros_like(t)) for t in G] + [torch.nn.Parameter(torch.zeros_like(gf)), pu]
    grads = G + [gf, gu]
    norm = math.sqrt(_sq64(grads))
    # two param groups: the norm is global over them too
    opt = AdamW([dict(params=params[:2]), dict(params=params[2:], weight_decay=0.0)], lr=1e-3, max_grad_norm=0.25 * norm)
    for p, gr in zip(params, grads):
        p.grad = gr
    opt.step()
    torch.cuda.synchronize()
    got = opt.last_grad_norm.item()
    assert abs(got - norm) <= 1e-5 * norm, (got, norm)
    coef = 0.25 * norm / (norm + 1e-6)
    for p, gr in zip(params, grads):
        m = opt.state[p]["exp_avg"].float()
        want = 0.1 * coef * gr.float()
        tol = 2 ** -7 if p.dtype == torch.bfloat16 else 1e-5   # two bf16 roundings / f32 arithmetic
        assert torch.allclose(m, want, rtol=tol, atol=1e-30), (p.dtype, (m - want).abs().max().item())


def test_nonfinite_norm_skips_the_step():
    from picotron_amd import _C
    from picotron_amd import kernels as K
    from picotron_amd.optim import AdamW
    K.device_status(torch.device(DEV))   # start from a clear word
    G = _grads()
    g = torch.Generator().manual_seed(8)
    gf = (torch.randn(3000, generator=g) * 0.3).to(DEV)
    P, M, V = _state()
    params = [torch.nn.Parameter(t.clone()) for t in P] + [torch.nn.Parameter(torch.randn(3000, generator=g).to(DEV))]
    opt = AdamW(params, lr=1e-3, max_grad_norm=1.0)
    for p, gr in zip(params, G + [gf]):
        p.grad = gr.clone()
    opt.step()   # a first finite step: the moments exist and are not zero
    torch.cuda.synchronize()
    assert K.device_status(torch.device(DEV)) == 0
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    params[2].grad.view(-1)[12345] = float("inf")
    opt.step()
    torch.cuda.synchronize()
    for p, (p0, m0, v0) in zip(params, before):
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]["exp_avg"], m0)
        assert torch.equal(opt.state[p]["exp_avg_sq"], v0)
    assert not math.isfinite(opt.last_grad_norm.item())
    with pytest.raises(_C.HipKernelError, match="gradient norm"):
        K.check_device_status(torch.device(DEV))
    # a following finite step updates normally, the status stays clear
    params[2].grad.view(-1)[12345] = 0.0
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(opt.last_grad_norm.item())
    for p, (p0, m0, v0) in zip(params, before):
        assert not torch.equal(p.detach(), p0) and not torch.equal(opt.state[p]["exp_avg"], m0)
    assert K.device_status(torch.device(DEV)) == 0
    K.check_device_status(torch.device(DEV))
    # the stand-alone clip on a NaN: gradients untouched, the same error
    params[0].grad[3] = float("nan")
    keep = [p.grad.clone() for p in params]
    from picotron_amd.optim import clip_grad_norm_
    total = clip_grad_norm_(params, 1.0)
    torch.cuda.synchronize()
    assert math.isnan(total.item())
    for p, k in zip(params, keep):
        assert torch.equal(p.grad.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32),
                           k.view(torch.int16 if p.dtype == torch.bfloat16 else torch.int32))
    with pytest.raises(_C.HipKernelError, match="gradient norm"):
        K.check_device_status(torch.device(DEV))


def test_clip_grad_norm_drop_in():
    """clip_grad_norm_ before the unclipped optimizer == AdamW(max_grad_norm), bit for bit; it
    returns the norm and scales f32 and unaligned gradients too."""
    from picotron_amd.optim import AdamW, clip_grad_norm_
    G = _grads()
    gf = _grads(dtype=torch.float32)[0] * 3
    P, _, _ = _state()
    norm = math.sqrt(_sq64(G + [gf]))
    a = [torch.nn.Parameter(t.clone()) for t in P] + [torch.nn.Parameter(torch.ones_like(gf))]
    b = [torch.nn.Parameter(t.clone()) for t in P] + [torch.nn.Parameter(torch.ones_like(gf))]
    for p, q, gr in zip(a, b, G + [gf]):
        p.grad, q.grad = gr.clone(), gr.clone()
    oa = AdamW(a, lr=1e-3, max_grad_norm=0.5 * norm)
    ob = AdamW(b, lr=1e-3)
    oa.step()
    total = clip_grad_norm_(b, 0.5 * norm)
    ob.step()
    torch.cuda.synchronize()
    assert total.dim() == 0 and total.is_cuda and abs(total.item() - norm) <= 1e-5 * norm
    assert torch.equal(total, oa.last_grad_norm)
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"])
        assert torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
    assert torch.allclose(b[-1].grad, gf * 0.5, rtol=1e-5)


# ------------------------------------------------------------------------------ multi-rank
def _reduction_body(rank, world):
    """tp2 x pp2, no model: sharded tensors differ per tp rank, replicated ones are equal across the
    tp pair, everything differs across pp.  The replicated tensors carry about 40 % of sq."""
    import torch.distributed as dist
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.optim import clip_grad_norm_
    torch.cuda.set_device(0)
    m = pgm.setup_process_group_manager(tp_size=2, cp_size=1, pp_size=2, dp_size=1)
    assert world == 4 and (m.pp_rank, m.tp_rank) == (rank // 2, rank % 2)

    def mk(seed, shape, scale, dtype=torch.bfloat16):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)
    # sharded: seeded by (pp, tp); replicated: by pp alone
    sh = [mk(100 + rank, (64, 1000), 0.1), mk(200 + rank, (1001,), 0.1), mk(300 + rank, (513,), 0.1, torch.float32)]
    rp = [mk(400 + m.pp_rank, (40000,), 0.15), mk(500 + m.pp_rank, (37,), 0.1), mk(600 + m.pp_rank, (99,), 0.1, torch.float32)]
    params = []
    for t, mark in [(x, True) for x in sh] + [(x, False) for x in rp]:
        p = torch.nn.Parameter(torch.zeros_like(t))
        p.grad = t.clone()
        if mark:
            p.tensor_model_parallel = True
        params.append(p)
    params = [params[0], params[3], params[1], params[4], params[2], params[5]]   # interleaved
    max_norm = 10.0
    total = clip_grad_norm_(params, max_norm)
    torch.cuda.synchronize()
    # gathered on the host: every shard and stage once, every replicated tensor once
    mine = torch.tensor([_sq64(sh), _sq64(rp), total.item()], dtype=torch.float64)
    every = [torch.zeros(3, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(every, mine)
    sq_sh = sum(e[0].item() for e in every)
    sq_rp = sum(every[r][1].item() for r in (0, 2))            # tp rank 0 of each stage
    assert every[0][1] == every[1][1] and every[2][1] == every[3][1] and every[0][1] != every[2][1]
    assert sq_rp >= 0.3 * (sq_sh + sq_rp), (sq_rp, sq_sh)       # counting them tp times: sqrt(1.3) off
    want = math.sqrt(sq_sh + sq_rp)
    assert abs(total.item() - want) <= 1e-5 * want, (total.item(), want)
    bits = torch.tensor([total.item()], dtype=torch.float64)
    allb = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(allb, bits)
    assert all(torch.equal(b, allb[0]) for b in allb)          # bit-equal on the four ranks
    # and every gradient was scaled by that one coefficient
    coef = max_norm / (want + 1e-6)
    for p, t in zip(params, [sh[0], rp[0], sh[1], rp[1], sh[2], rp[2]]):
        tol = 2 ** -8 if t.dtype == torch.bfloat16 else 1e-5
        assert torch.allclose(p.grad.float(), t.float() * coef, rtol=tol, atol=1e-30)


def test_norm_reduction_tp2_pp2():
    _dist.run(_reduction_body, 4, device="cuda")


def _tp2_llama_body(rank, world):
    import torch.distributed as dist
    from picotron_amd import functional as FN
    from picotron_amd.optim import AdamW
    from tests.test_parallel_gpu import CFG, TOL, _rel, _setup, _shard
    m, model, names, pf, ids, lo, loss_r = _setup(2, 1)
    assert all(layer.tp_sequence_parallel for layer in model.decoder_layers)   # the default
    V = CFG["vocab_size"]
    logits = model(ids[:, :-1].cuda())
    loss = FN.cross_entropy(logits.view(-1, V), ids[:, 1:].reshape(-1).cuda())
    loss.backward()
    oracle_norm = math.sqrt(sum(pf[n].grad.double().pow(2).sum().item() for n in names))
    n_sharded = 0
    for n, p in names.items():   # sharded <=> marked
        sharded = tuple(p.shape) != tuple(pf[n].shape)
        assert bool(getattr(p, "tensor_model_parallel", False)) == sharded, n
        n_sharded += sharded
    assert 0 < n_sharded < len(names)
    max_norm = 0.25 * oracle_norm
    opt = AdamW(model.parameters(), max_grad_norm=max_norm)
    opt.step()
    torch.cuda.synchronize()
    got = opt.last_grad_norm.item()
    assert abs(got - oracle_norm) < TOL * oracle_norm, (got, oracle_norm)
    both = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, torch.tensor([got], dtype=torch.float64))
    assert torch.equal(both[0], both[1])
    coef_hip = min(1.0, max_norm / (got + 1e-6))
    assert coef_hip < 0.3
    for n, p in names.items():
        want = 0.1 * coef_hip * _shard(pf[n].grad, p, m.tp_rank)
        assert _rel(opt.state[p]["exp_avg"], want) < TOL, n


def test_tp2_llama_clipped_step():
    _dist.run(_tp2_llama_body, 2, device="cuda")
