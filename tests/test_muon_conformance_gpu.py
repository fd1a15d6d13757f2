"""Muon on the GPU, stage by stage (csrc/muon.hip, kernels.muon_newton_schulz) against tests/_muon_ref.py:
the momentum, scale and apply kernels per element on multi-tensor lists, the per-tensor squared
norms, every Newton-Schulz iteration's A, S, P' and X on the chain's own intermediates, and the
iteration end to end beside torch's own bf16 iteration."""
import pytest
import torch

from tests import _muon_ref as M

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32

# A list whose lengths straddle the 8-element chunk (63, 16383) and the 2048-chunk block (16383 <
# 16384 < 16512 < 2 * 16384 < 33280), with ragged tails (63, 16383), column counts off the 8-grid
# (7, 127, 129: the scalar form inside a list) and images off the 64-grid.
LIST_SHAPES = [(24, 40), (9, 7), (129, 127), (64, 64), (128, 129), (72, 40), (130, 256)]


def _mk(shape, seed, gdtype, gscale=1.0, **kw):
    gen = torch.Generator().manual_seed(4242 + seed)
    R, C = shape
    p = (torch.randn(R, C, generator=gen) * 0.02).to(BF)
    g = (M.make_grad("gauss", R, C, seed).float() * gscale).to(gdtype)
    buf = (torch.randn(R, C, generator=gen) * 0.01 * gscale).to(gdtype)
    return M.Case(p, g, buf, **kw)


def _list(gdtype, **kw):
    cases = [_mk(s, i, gdtype, **kw) for i, s in enumerate(LIST_SHAPES)]
    cases.append(_mk((24, 40), 50, gdtype, gscale=0.0, **kw))      # zero gradient and buffer
    cases.append(_mk((24, 40), 51, gdtype, gscale=5e-7, **kw))     # ||u|| of the order of eps: the clamp
    return cases


def _device_items(cases, place=None):
    """place(name, cpu tensor) -> device tensor; default: a fresh aligned copy"""
    from picotron_amd import kernels as K
    place = place or (lambda name, t: t.to(DEV).clone())
    return [(place("p", c.p), place("g", c.g), place("buf", c.buf), K.muon_x_workspace(c.p.shape, DEV),
             K.muon_lr_ratio(c.adjust, c.p.shape)) for c in cases]


def _run(cases, clip=None, place=None):
    """The whole step on a list of cases that share their hyper-parameters; [check_step's out]."""
    from picotron_amd import kernels as K
    items = _device_items(cases, place)
    c0 = cases[0]
    sq = K.muon_momentum(items, c0.mu, c0.nesterov, clip=clip)
    K.muon_scale(items, sq, c0.mu, c0.nesterov, c0.eps, clip=clip)
    st = {}
    K.muon_newton_schulz([it[3] for it in items], c0.coeffs, c0.ns_steps, stages=st)
    K.muon_apply(items, c0.lr, c0.wd, clip=clip)
    torch.cuda.synchronize()
    sq = sq.cpu()
    return [dict(buf=it[2].cpu(), sq=float(sq[i]), sq_bits=sq[i].clone(), X0=st["X0"][i].cpu(), p=it[0].cpu(),
                 iters=[{k: rec[k][i].cpu() for k in "ASPX"} for rec in st["iters"]]) for i, it in enumerate(items)]


def _same_bits(a, b, what):
    for k in ("buf", "sq_bits", "X0", "p"):
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32 if x.dtype == F32 else torch.int16),
                                                  y.view(torch.int32 if y.dtype == F32 else torch.int16)), f"{what}: {k}"


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("mu", [0.95, 0.25])
@pytest.mark.parametrize("gdtype", [BF, F32], ids=["bf16", "f32"])
def test_list_step_per_element(gdtype, mu, nesterov):
    """momentum, squared norm, scale, two iterations and the apply of a mixed list, every stage of every
    tensor; mu on both sides of 0.5 takes both forms of lerp in both places."""
    kw = dict(momentum=mu, nesterov=nesterov, ns_steps=2, lr=0.02, weight_decay=0.1)
    cases = _list(gdtype, **kw)
    if gdtype == F32 and not nesterov and mu == 0.25:   # the adversarial family of lerp's w >= 0.5 form
        g, buf = M.cancel_case(24, 40)
        cases.append(M.Case(torch.zeros(24, 40, dtype=BF), g, buf, **kw))
    outs = _run(cases)
    for i, (c, o) in enumerate(zip(cases, outs)):
        M.check_step(c, o, tag=f"t{i} {c.R}x{c.C} ")
    zero = outs[len(LIST_SHAPES)]
    cz = cases[len(LIST_SHAPES)]
    assert float(zero["X0"].float().abs().max()) == 0.0 and zero["sq"] == 0.0
    assert torch.equal(zero["p"], (cz.p.float() * torch.tensor(1 - cz.lr * cz.wd, dtype=F32)).to(BF))


@pytest.mark.parametrize("adjust", ["original", "match_rms_adamw"])
def test_apply_lr_adjustment(adjust):
    cases = [_mk(s, i, BF, ns_steps=1, adjust_lr_fn=adjust) for i, s in enumerate([(72, 40), (24, 40)])]
    for c, o in zip(cases, _run(cases)):
        M.check_step(c, o, tag=f"{adjust} {c.R}x{c.C} ")


@pytest.mark.parametrize("gdtype", [BF, F32], ids=["bf16", "f32"])
def test_scalar_form_gives_the_vector_forms_bits(gdtype):
    """Every tensor 2 bytes (bf16) / 4 bytes (f32) past a 16-byte boundary, and as a column slice of a
    wider tensor (a row stride): the element-by-element form, the same bits as the aligned list.  And as a
    16-byte-aligned column slice whose row stride is a multiple of 8 above the column count: the VECTOR
    form through a row stride (shapes with C % 8 == 0; the others stay element by element), the same
    bits again."""
    cases = [_mk(s, i, gdtype, ns_steps=1) for i, s in
             enumerate([(24, 40), (9, 7), (129, 127), (64, 64), (130, 256)])]
    want = _run(cases)

    def unaligned(name, t):
        base = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
        v = base[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0
        return v

    def strided(name, t):
        base = torch.zeros(t.shape[0], t.shape[1] + 3, dtype=t.dtype, device=DEV)
        v = base[:, 1:1 + t.shape[1]]
        v.copy_(t)
        return v
    def strided_vec(name, t):
        base = torch.zeros(t.shape[0], -(-t.shape[1] // 8) * 8 + 16, dtype=t.dtype, device=DEV)
        v = base[:, 8:8 + t.shape[1]]
        v.copy_(t)
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0 and v.stride(0) > t.shape[1]
        return v
    for place in (unaligned, strided, strided_vec):
        got = _run(cases, place=place)
        for i, (a, b) in enumerate(zip(got, want)):
            _same_bits(a, b, f"{place.__name__} t{i}")


def test_squared_norms_reproducible_and_position_independent():
    """A tensor's squared norm has the same bits on a second run and wherever it stands in the list."""
    cases = _list(BF, ns_steps=0)
    a, b = _run(cases), _run(cases)
    order = list(range(len(cases)))[::-1]
    order = order[3:] + order[:3]
    r = _run([cases[i] for i in order])
    for i, c in enumerate(cases):
        M.check_sq(c, a[i]["buf"], a[i]["sq"], tag=f"t{i} ")
        _same_bits(a[i], b[i], f"second run t{i}")
        _same_bits(a[i], r[order.index(i)], f"moved t{i}")


def test_clip_variants():
    """CLIP: coef < 1 per element; coef = 1 the unclipped bits; a non-finite norm writes nothing and
    raises the status bit."""
    from picotron_amd import kernels as K
    dev = torch.device(DEV)
    K.device_status(dev)
    for gdtype in (BF, F32):
        plain = [_mk(s, i, gdtype, ns_steps=1) for i, s in enumerate([(24, 40), (9, 7), (129, 127)])]
        gsq = torch.tensor([4.0], dtype=F32, device=DEV)
        coef = M.clip_coef32(4.0, 1.0)
        assert coef < 1
        clipped = [M.Case(c.p, c.g, c.buf, ns_steps=1, coef=coef) for c in plain]
        for c, o in zip(clipped, _run(clipped, clip=(gsq, 1.0, None))):
            M.check_step(c, o, tag=f"clip {c.R}x{c.C} ")
        one = _run(plain, clip=(torch.tensor([0.25], dtype=F32, device=DEV), 1.0, None))
        for i, (a, b) in enumerate(zip(one, _run(plain))):
            _same_bits(a, b, f"coef 1 t{i}")
        assert K.device_status(dev) == 0
        # non-finite: nothing is written
        items = _device_items(plain)
        keep = [(it[0].clone(), it[2].clone()) for it in items]
        for it in items:
            it[3].fill_(0.125)   # a stale image: the apply must not consume it
        bad = (torch.tensor([float("inf")], dtype=F32, device=DEV), 1.0, K.status_word(dev))
        sq = K.muon_momentum(items, 0.95, True, clip=bad)
        K.muon_scale(items, sq, 0.95, True, 1e-7, clip=bad)
        K.muon_apply(items, 0.02, 0.1, clip=bad)
        torch.cuda.synchronize()
        for it, (p0, b0) in zip(items, keep):
            assert torch.equal(it[0], p0) and torch.equal(it[2], b0)
            assert float((it[3] - 0.125).abs().max()) == 0.0
        assert K.device_status(dev) & K.STATUS_NONFINITE_GRAD


NS_SHAPES = [(64, 64), (64, 192), (192, 64), (128, 320), (72, 40)]


def _ns(us, ns_steps=5):
    """X0 = bf16(u / ||u||) on the CPU into images, the iteration on the device; (stages, results)."""
    from picotron_amd import kernels as K
    xs = []
    for u in us:
        x = K.muon_x_workspace(u.shape, DEV)
        x[:u.shape[0], :u.shape[1]] = (u.double() / u.double().norm()).to(BF).to(DEV)
        xs.append(x)
    st = {}
    K.muon_newton_schulz(xs, M.NS_COEFFS, ns_steps, stages=st)
    torch.cuda.synchronize()
    return st, [x.cpu() for x in xs]


@pytest.mark.parametrize("shape", NS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_newton_schulz_stage_by_stage(shape):
    R, C = shape
    u = M.make_grad("gauss", R, C, 3)
    c = M.Case(torch.zeros(R, C, dtype=BF), u, torch.zeros(R, C, dtype=BF))
    st, out = _ns([u])
    X = st["X0"][0].cpu()
    for k, rec in enumerate(st["iters"]):
        M.check_iteration(c, X, {n: rec[n][0] for n in "ASPX"}, f"{R}x{C} it{k} ")
        X = rec["X"][0].cpu()
    assert torch.equal(X, out[0])   # O is left in the matrix's own image


def test_newton_schulz_groups_of_four_plus_one():
    """5 matrices of 64x128 in one call: a launch of 4 and a launch of 1; each result bit-equal to the
    matrix run alone."""
    from picotron_amd import kernels as K
    assert [len(idx) for _, idx in K.muon_group_plan([(64, 128)] * 5)] == [4, 1]
    us = [M.make_grad("gauss", 64, 128, 10 + i) for i in range(5)]
    _, together = _ns(us)
    for i, u in enumerate(us):
        _, alone = _ns([u])
        assert torch.equal(together[i].view(torch.int16), alone[0].view(torch.int16)), f"matrix {i}"


@pytest.mark.parametrize("kind", ["gauss", "colscaled"])
def test_newton_schulz_end_to_end(kind):
    """||O_hip - O64|| / ||O64|| <= 2 x the same figure of torch's bf16 iteration on the CPU (O64: the
    float64 iteration without roundings).  Why 2: both iterations round to bf16 at the same number of
    points (A, the polynomial, X per iteration), so their errors are of one size; folding a I into P' measured at
    most 1.35x torch's figure on the CPU emulator at these shapes, and the GEMMs' f32 summation order differs."""
    us = [M.make_grad(kind, R, C, 1) for R, C in NS_SHAPES]
    _, outs = _ns(us)
    for (R, C), u, o in zip(NS_SHAPES, us, outs):
        o64 = M.ns_f64(u.double())
        ours, theirs = M.fro_rel(o[:R, :C], o64), M.fro_rel(M.ns_torch_bf16(u), o64)
        print(f"muon-ns {kind} {R}x{C}: hip {ours:.5f} torch-bf16 {theirs:.5f} ratio {ours / theirs:.2f}")
        assert ours <= 2 * theirs, (kind, R, C, ours, theirs)
