"""kernels.moe_route_sigmoid / moe_route_sigmoid_bwd / moe_bias_update against tests/_moe_sigmoid_ref.py
(float64) with the bounds tests/_moe_ref.py applies to the softmax router's same outputs: idx and counts
exact, gate / probs / aux within F32_TOL, dlogits within one bf16 ulp plus the propagated f32 allowance."""
import itertools

import pytest
import torch

from tests import _moe_ref as R
from tests import _moe_sigmoid_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(8, 1, 1, 2), (16, 4, 2, 4), (64, 8, 3, 6), (128, 8, 4, 8), (96, 1, 1, 8), (128, 4, 2, 8)]
GRID = [(256, None) + c + v for c in CASES for v in itertools.product((0, 1), (1.0, 2.5), (False, True))]
GRID.append((37, 72, 64, 8, 3, 6, 1, 2.5, True))   # ragged: the last workgroup half empty, ldl > E


def _route(logits, bias, k, G, Kg, norm, scale, load=None):
    from picotron_amd import kernels as K
    dev = torch.empty(logits.shape[0], logits.stride(0), dtype=R.BF, device=DEV)[:, :logits.shape[1]]   # keeps ldl
    return K.moe_route_sigmoid(dev.copy_(logits), k, norm, None if bias is None else bias.to(DEV), G, Kg, scale, load)


@pytest.mark.parametrize("T,ldl,E,G,Kg,k,norm,scale,use_bias", GRID)
def test_route_and_backward_against_float64(T, ldl, E, G, Kg, k, norm, scale, use_bias):
    from picotron_amd import kernels as K
    for seed in range(5):
        logits, bias, dgate, d_aux = S.inputs(T, E, k, seed, ldl)
        bias = bias if use_bias else None
        idx, gate, probs, counts, aux = _route(logits, bias, k, G, Kg, norm, scale)
        ref_idx, _, _, _, _, margin = S.ref_route(logits, bias, k, G, Kg, norm, scale)
        ok = margin >= S.MARGIN
        assert int((~ok).sum()) <= S.MAX_EXCLUDED * T, f"{int((~ok).sum())} of {T} tokens under the margin"
        R.check_exact("idx", idx.cpu()[ok], ref_idx[ok])
        _, ref_gate, s, ref_counts, ref_aux, _ = S.ref_route(logits, bias, k, G, Kg, norm, scale, idx=idx.cpu())
        R.check_exact("counts", counts, ref_counts)
        R.check_rel("gate", gate.cpu()[ok], ref_gate[ok])
        R.check_rel("probs", probs.cpu()[ok], s[ok])
        R.check_rel("aux", aux, ref_aux)
        dl = K.moe_route_sigmoid_bwd(dgate.to(DEV), probs, idx, gate, counts, d_aux.to(DEV), norm, scale)
        ref_dl, allow = S.ref_route_bwd(logits, idx.cpu(), dgate, d_aux, norm, scale, R.F32_TOL)
        R.check_bf16("dlogits", dl, ref_dl, extra=allow)


def test_two_launches_give_identical_bits_and_padded_columns_are_zero():
    from picotron_amd import kernels as K
    logits, bias, dgate, d_aux = S.inputs(256, 128, 8, 0)
    runs = []
    for _ in range(2):
        out = _route(logits, bias, 8, 8, 4, 1, 2.5)
        runs.append(out + (K.moe_route_sigmoid_bwd(dgate.to(DEV), out[2], out[0], out[1], out[3], d_aux.to(DEV), 1, 2.5),))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16) if a.dtype == R.BF else a, b.view(torch.int16) if b.dtype == R.BF else b)
    lib, (idx, gate, probs, counts, _, _) = K._C.lib(), runs[0]   # the C entry on a padded row: columns E.. must be +0
    wide = torch.full((256, 136), 7.0, dtype=R.BF, device=DEV)
    rc = lib.pt_moe_route_sigmoid_bwd(dgate.to(DEV).data_ptr(), probs.data_ptr(), idx.data_ptr(), gate.data_ptr(),
                                      counts.data_ptr(), None, 1, 2.5, wide.data_ptr(), 136, 256, 128, 8, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((wide[:, 128:].view(torch.int16) == 0).all()) and not bool((wide[:, :128] == 7.0).all())


@pytest.mark.parametrize("designed", [False, True])
def test_bias_update_on_an_accumulated_load(designed):
    """load accumulates over two route calls; the step equals torch's f32 bias + rate * sign exactly and
    clears load.  designed: one-hot logits with counts (2, 2, 3, 1) -- experts 0 and 1 sit at the mean and
    keep their bias (the route call itself runs without the bias there, so the counts are the designed ones)."""
    from picotron_amd import kernels as K
    if designed:
        E, k, args = 4, 1, (1, 1, 1, 1.0)
        logits = torch.full((8, E), -4.0)
        logits[torch.arange(8), torch.tensor([0, 0, 1, 1, 2, 2, 2, 3])] = 4.0
        logits, bias = logits.to(R.BF), torch.tensor([0.25, -0.5, 0.0, 1.0])
    else:
        E, k, args = 64, 6, (8, 3, 1, 1.0)
        logits, bias, _, _ = S.inputs(256, E, k, 1)
    load, dbias, rate = torch.zeros(E, dtype=torch.int32, device=DEV), bias.to(DEV), 1e-3
    for _ in range(2):
        counts = _route(logits, None if designed else bias, k, *args, load=load)[3]
    assert torch.equal(load, 2 * counts)
    lc = load.cpu().long()
    want = bias + rate * torch.sign(lc.sum() - E * lc).to(torch.float32)
    K.moe_bias_update(dbias, load, rate)
    assert torch.equal(dbias.cpu(), want) and not bool(load.any())
    if designed:
        assert lc.tolist() == [4, 4, 6, 2] and torch.equal(dbias.cpu()[:2], bias[:2]) and not torch.equal(dbias.cpu(), bias)
