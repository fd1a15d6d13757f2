"""The Muon conformance kit checks itself (CPU): tests/_muon_ref.py's checker accepts the clean
emulator of the step on every case and rejects each injected fault, on a case built to show it."""
import pytest
import torch

from tests import _muon_ref as M

BF, F32 = torch.bfloat16, torch.float32


def _case(R, C, seed=0, gscale=1.0, pscale=1.0, gdtype=BF, **kw):
    gen = torch.Generator().manual_seed(1000 + seed)
    p = (torch.randn(R, C, generator=gen) * 0.02 * pscale).to(BF)
    g = (M.make_grad("gauss", R, C, seed).float() * gscale).to(gdtype)
    buf = (torch.randn(R, C, generator=gen) * 0.01 * gscale).to(gdtype)
    return M.Case(p, g, buf, **kw)


def _cancel():
    g, buf = M.cancel_case(24, 40)
    p = torch.zeros(24, 40, dtype=BF)
    return M.Case(p, g, buf, momentum=0.25, nesterov=False)


CASES = {
    "wide": lambda: _case(24, 40),
    "tall": lambda: _case(72, 40, seed=1, lr=0.02, adjust_lr_fn=None),
    "tall_rms": lambda: _case(72, 40, seed=2, adjust_lr_fn="match_rms_adamw"),
    "ragged": lambda: _case(9, 7, seed=3),
    "tiny": lambda: _case(24, 40, seed=4, gscale=5e-7),
    "zero": lambda: _case(24, 40, seed=5, gscale=0.0),
    "f32": lambda: _case(24, 40, seed=6, gdtype=F32, momentum=0.3, nesterov=False),
    "plain": lambda: _case(64, 64, seed=7, nesterov=False, ns_steps=2),
    "clipped": lambda: _case(24, 40, seed=8, coef=M.clip_coef32(4.0, 1.0)),
    "cancel": _cancel,
    "big_step": lambda: _case(24, 40, seed=9, lr=0.5, weight_decay=0.5, pscale=0.5),
}
# fault -> the case that shows it.  norm_unrounded needs u known exactly (f32 buffers, no Nesterov:
# u = bf16(buf)): with momentum 0.95 a few percent of the Nesterov u sit on bf16 ties (0.95 k is a half-
# integer for every k = 10 mod 20) and the squared norm's interval is as wide as the fault's effect.
FAULT_CASE = {"lerp_branch": "cancel", "norm_unrounded": "f32", "eps_added": "tiny", "diag_missing": "wide",
              "a_whole_row": "wide", "s_bf16": "wide", "untransposed_gram": "tall", "decay_after": "big_step",
              "lr_unadjusted": "tall", "tail_dropped": "ragged"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_clean_emulator_is_accepted(name):
    c = CASES[name]()
    out = M.emu_step(c)
    M.check_step(c, out, tag=f"{name} ")
    if name == "zero":   # X0 = 0: the parameter only decays, nothing is NaN
        assert float(out["X0"].float().abs().max()) == 0.0
        assert torch.equal(out["p"], (c.p.float() * torch.tensor(1 - c.lr * c.wd, dtype=F32)).to(BF))


def test_every_fault_has_a_case():
    assert sorted(FAULT_CASE) == sorted(M.FAULTS)


@pytest.mark.parametrize("fault", M.FAULTS)
def test_fault_is_rejected(fault):
    c = CASES[FAULT_CASE[fault]]()
    with pytest.raises(AssertionError):
        M.check_step(c, M.emu_step(c, fault=fault), tag=f"{fault} ")


def test_fold_against_torch_bf16():
    """The folded iteration's distance to the float64 iteration, beside torch's own bf16 iteration's
    (both round to bf16 at the same number of points, so the two are of one size: within 2x)."""
    for kind in ("gauss", "colscaled"):
        for R, C in ((64, 64), (64, 192), (192, 64)):
            u = M.make_grad(kind, R, C)
            c = M.Case(torch.zeros(R, C, dtype=BF), u, torch.zeros(R, C, dtype=BF), momentum=0.0, nesterov=False)
            o = M.emu_step(c)["iters"][-1]["X"][:R, :C]
            o64 = M.ns_f64(u.double())
            ours, theirs = M.fro_rel(o, o64), M.fro_rel(M.ns_torch_bf16(u), o64)
            print(f"fold {kind} {R}x{C}: emulator {ours:.4f} torch bf16 {theirs:.4f}")
            assert ours <= 2 * theirs
