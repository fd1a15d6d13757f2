"""The host side of the z-loss entry points (csrc/cross_entropy.hip's _z functions) and of the Python
keywords, without a GPU: the real library loads on a machine with no device and its argument checks return
before any HIP call.  Pointers are fake, non-null, 16-byte-aligned integers (never dereferenced: every call
here is refused)."""
import math

import pytest
import torch

PT_EINVAL, PT_EALIGN = -1, -2
P = [0x10000000 + i * 0x100000 for i in range(10)]   # fake device pointers

# entry -> its arguments in ABI order, the stream (NULL) appended by call()
DEFAULTS = {
    "pt_cross_entropy_fwd_bwd_z": dict(logits=P[0], logits_stride=64, targets=P[1], dlogits=P[2], dlogits_stride=64,
                                       row_loss=P[3], rows=4, vocab=64, scale=1.0, inv_count=None, ignore_index=-100,
                                       status=None, z_coef=0.25, row_z=P[8]),
    "pt_cross_entropy_fwd_lse_z": dict(logits=P[0], logits_stride=64, targets=P[1], row_loss=P[3], row_lse=P[4], rows=4,
                                       vocab=64, ignore_index=-100, status=None, z_coef=0.25, row_z=P[8]),
    "pt_cross_entropy_bwd_lse_z": dict(logits=P[0], logits_stride=64, targets=P[1], row_lse=P[4], dlogits=P[2],
                                       dlogits_stride=64, rows=4, vocab=64, scale=P[5], scale_stride=0,
                                       ignore_index=-100, z_coef=0.25),
    "pt_cross_entropy_bwd_lse_shard_z": dict(logits=P[0], logits_stride=64, targets=P[1], row_lse=P[4], dlogits=P[2],
                                             dlogits_stride=64, rows=4, vocab_shard=64, vocab_lo=64, scale=P[5],
                                             scale_stride=0, ignore_index=-100, z_coef=0.25),
    "pt_cross_entropy_fwd_stats_z": dict(logits=P[0], logits_stride=64, targets=P[1], stats=P[6], nblk=2, row_loss=P[3],
                                         row_lse=P[4], rows=4, vocab=64, ignore_index=-100, status=None, z_coef=0.25,
                                         row_z=P[8]),
    "pt_cross_entropy_vp_combine_z": dict(parts=P[7], tp=2, targets=P[1], row_loss=P[3], row_lse=P[4], rows=4, vocab=128,
                                          ignore_index=-100, status=None, z_coef=0.25, row_z=P[8]),
}
# the pointers each entry point requires (row_z, status and inv_count are optional)
REQUIRED = {
    "pt_cross_entropy_fwd_bwd_z": ("logits", "targets", "row_loss"),
    "pt_cross_entropy_fwd_lse_z": ("logits", "targets", "row_loss", "row_lse"),
    "pt_cross_entropy_bwd_lse_z": ("logits", "targets", "row_lse", "dlogits", "scale"),
    "pt_cross_entropy_bwd_lse_shard_z": ("logits", "targets", "row_lse", "dlogits", "scale"),
    "pt_cross_entropy_fwd_stats_z": ("logits", "targets", "stats", "row_loss", "row_lse"),
    "pt_cross_entropy_vp_combine_z": ("parts", "targets", "row_loss", "row_lse"),
}


def lib():
    from tests.test_row_host_cpu import library
    return library()


def call(entry, **over):
    a = dict(DEFAULTS[entry])
    assert not set(over) - set(a), (entry, over)
    a.update(over)
    return getattr(lib(), entry)(*a.values(), None)


def test_every_z_entry_point_is_bound():
    from picotron_amd import _C
    assert set(DEFAULTS) == {n for n in _C.SIGNATURES if n.startswith("pt_cross_entropy") and n.endswith("_z")}
    for n in DEFAULTS:
        assert n[:-2] in _C.SIGNATURES, f"{n} has no plain namesake"
        assert len(_C.SIGNATURES[n][1]) == len(DEFAULTS[n]) + 1


@pytest.mark.parametrize("entry", sorted(DEFAULTS))
@pytest.mark.parametrize("z", [-1.0, math.nan, math.inf, -math.inf, -1e-30])
def test_bad_coefficient_is_refused(entry, z):
    assert call(entry, z_coef=z) == PT_EINVAL


@pytest.mark.parametrize("entry", sorted(DEFAULTS))
def test_bad_coefficient_answers_before_every_other_check(entry):
    """z_coef is checked first: with a misaligned pointer as well the answer is PT_EINVAL, not PT_EALIGN."""
    first = "parts" if entry.endswith("combine_z") else "stats" if entry.endswith("stats_z") else "logits"
    assert call(entry, **{first: P[0] + 8}) == (PT_EINVAL if first == "stats" else PT_EALIGN)
    assert call(entry, z_coef=-1.0, **{first: P[0] + 8}) == PT_EINVAL


@pytest.mark.parametrize("entry", sorted(DEFAULTS))
def test_null_pointers_are_refused(entry):
    for z in (0.25, 0.0):
        for name in REQUIRED[entry]:
            assert call(entry, z_coef=z, **{name: None}) == PT_EINVAL, (entry, name, z)
    assert call(entry, rows=0) == PT_EINVAL


@pytest.mark.parametrize("z", [-1.0, -0.25, math.nan, math.inf, -math.inf, 1e39])
def test_functional_rejects_bad_z_loss(z):
    from picotron_amd import functional as FN
    x, t = torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        FN.cross_entropy(x, t, z_loss=z)
    with pytest.raises(ValueError):
        FN.cross_entropy(x, t, z_loss=z, return_z_loss=True)


def test_wrappers_and_steps_take_the_keyword():
    """Every layer the coefficient passes through names it (a ValueError, not a TypeError, for a bad value)."""
    import inspect
    from picotron_amd import kernels as K, train
    from picotron_amd.pipeline_parallel import pipeline_parallel as PP
    for fn in (K.cross_entropy_loss_lse, K.cross_entropy_loss_lse_stats, K.cross_entropy_vp_combine,
               K.cross_entropy_grad_lse, K.cross_entropy_grad_lse_shard, K.cross_entropy_fwd_bwd, train.train_step,
               train.GraphedTrainStep.__init__, PP.train_step_pipeline_afab, PP.train_step_pipeline_1f1b):
        par = inspect.signature(fn).parameters
        assert "z_loss" in par and par["z_loss"].default == 0.0, fn
    assert K.z_coef(1e-4) == float(torch.tensor(1e-4, dtype=torch.float32)) and K.z_coef(0) == 0.0
    for bad in (-1.0, math.nan, math.inf, "0.1", None, True):
        with pytest.raises(ValueError):
            K.z_coef(bad)
    # not a Python float: the message names the type
    with pytest.raises(ValueError, match="Tensor"):
        K.z_coef(torch.tensor(0.25))
    assert K.z_coef(float(torch.tensor(0.25))) == 0.25
