"""Global gradient-norm clipping, the parts that need no device: how the norm is put together on a
(tp, pp) grid (optim.grad_norm_plan), argument checks of the Python interface, and the new C-ABI
entry points' argument errors."""
import ctypes
import types

import pytest


def _fake(name, marked):
    p = types.SimpleNamespace(name=name)
    if marked:
        p.tensor_model_parallel = True
    return p


@pytest.mark.parametrize("tp,pp,groups", [(1, 1, ()), (2, 1, ("tp",)), (1, 2, ("pp",)), (2, 2, ("tp", "pp"))])
def test_grad_norm_plan(tp, pp, groups):
    from picotron_amd.optim import grad_norm_plan
    params = [_fake("embedding.weight", True), _fake("norm.weight", False), _fake("q_proj.weight", True),
              _fake("out_proj.bias", False), _fake("out_proj.weight", True)]
    params[3].tensor_model_parallel = False   # an explicit False is no mark either
    sharded, replicated, g, w = grad_norm_plan(params, tp, pp)
    # a partition, in order, by the mark alone
    assert [p.name for p in sharded] == ["embedding.weight", "q_proj.weight", "out_proj.weight"]
    assert [p.name for p in replicated] == ["norm.weight", "out_proj.bias"]
    assert g == groups
    assert w == 1.0 / tp
    # sum over the tp ranks of sq(sharded) + w * sq(replicated) counts a replicated tensor once
    assert tp * w == 1.0


def test_grad_norm_plan_rejects_bad_grid():
    from picotron_amd.optim import grad_norm_plan
    with pytest.raises(ValueError):
        grad_norm_plan([], 0, 1)


@pytest.mark.parametrize("norm_type", [1.0, float("inf"), 3])
def test_clip_grad_norm_l2_only(norm_type):
    import torch
    from picotron_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError):
        clip_grad_norm_([p], 1.0, norm_type=norm_type)
    assert torch.equal(p.grad, torch.ones(4))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_adamw_rejects_bad_max_grad_norm(bad):
    import torch
    from picotron_amd.optim import AdamW
    with pytest.raises(ValueError):
        AdamW([torch.nn.Parameter(torch.ones(4))], max_grad_norm=bad)
    assert AdamW([torch.nn.Parameter(torch.ones(4))]).max_grad_norm is None
    assert AdamW([torch.nn.Parameter(torch.ones(4))], max_grad_norm=1).max_grad_norm == 1.0


def test_status_bit_matches_header():
    import os
    import re
    from picotron_amd import kernels as K
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "picotron_hip.h")).read()
    assert int(re.search(r"#define PT_STATUS_NONFINITE_GRAD (\d+)", txt).group(1)) == K.STATUS_NONFINITE_GRAD == 2


def test_grad_clip_abi_argument_errors():
    """Null pointers, negative counts and a max_norm that is not positive return PT_EINVAL (-1) before
    any launch (no device needed); the workspace query returns a count."""
    from picotron_amd import _C
    lib = _C.load_library()
    assert lib.pt_grad_sq_workspace() > 0
    buf = (ctypes.c_float * 8)()
    a = ctypes.addressof(buf)   # a non-null pointer that is never dereferenced: every call below fails first
    sc = (0.999, 0.1, 0.999, 0.001, 0.03, 1e-8, -3e-4)
    # sum of squares, list form: table, chunk_start, ntensors, total_chunks, weight, accumulate, workspace, sq
    assert lib.pt_grad_sq_multi(None, a, 1, 1, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq_multi(a, None, 1, 1, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq_multi(a, a, 0, 1, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq_multi(a, a, 1, -1, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq_multi(a, a, 1, 1, 1.0, 0, None, a, None) == -1
    assert lib.pt_grad_sq_multi(a, a, 1, 1, 1.0, 0, a, None, None) == -1
    # single tensor: grad, n, dtype, weight, accumulate, workspace, sq
    assert lib.pt_grad_sq(None, 8, 0, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq(a, -1, 0, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq(a, 8, 2, 1.0, 0, a, a, None) == -1
    assert lib.pt_grad_sq(a, 8, 0, 1.0, 0, None, a, None) == -1
    assert lib.pt_grad_sq(a, 8, 0, 1.0, 0, a, None, None) == -1
    # in-place scale
    assert lib.pt_grad_scale_multi(None, a, 1, 1, a, 1.0, None, None) == -1
    assert lib.pt_grad_scale_multi(a, a, 1, -1, a, 1.0, None, None) == -1
    assert lib.pt_grad_scale_multi(a, a, 1, 1, None, 1.0, None, None) == -1
    assert lib.pt_grad_scale_multi(a, a, 1, 1, a, 0.0, None, None) == -1
    assert lib.pt_grad_scale(None, 8, 0, a, 1.0, None, None) == -1
    assert lib.pt_grad_scale(a, -8, 0, a, 1.0, None, None) == -1
    assert lib.pt_grad_scale(a, 8, 0, None, 1.0, None, None) == -1
    assert lib.pt_grad_scale(a, 8, 0, a, -1.0, None, None) == -1
    assert lib.pt_grad_scale(a, 8, 7, a, 1.0, None, None) == -1
    # clipped AdamW
    assert lib.pt_adamw_step_clip(None, a, a, a, 8, 0, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_clip(a, a, a, a, -1, 0, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_clip(a, a, a, a, 8, 0, *sc, None, 1.0, None, None) == -1
    assert lib.pt_adamw_step_clip(a, a, a, a, 8, 0, *sc, a, 0.0, None, None) == -1
    assert lib.pt_adamw_step_clip(a, a, a, a, 8, 3, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(None, a, 1, 1, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(a, None, 1, 1, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(a, a, 0, 1, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(a, a, 1, -1, *sc, a, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(a, a, 1, 1, *sc, None, 1.0, None, None) == -1
    assert lib.pt_adamw_step_multi_clip(a, a, 1, 1, *sc, a, float("nan"), None, None) == -1


_SC = (0.999, 0.1, 0.999, 0.001, 0.03, 1e-8, -3e-4)
_P = 16   # any non-null address: every call below returns before a pointer is read


def test_unclipped_step_abi_argument_errors():
    """pt_adamw_step and pt_adamw_step_multi: PT_EINVAL (-1) for a NULL pointer, a negative count and
    an unknown dtype, PT_OK (0) for nothing to do -- but only with valid arguments: an unknown dtype
    is refused at n == 0 as well, as every sibling entry does."""
    from picotron_amd import _C
    lib = _C.load_library()
    for i in range(4):   # param, grad, exp_avg, exp_avg_sq
        ptrs = [_P] * 4
        ptrs[i] = None
        assert lib.pt_adamw_step(*ptrs, 8, 0, *_SC, None) == -1
    assert lib.pt_adamw_step(_P, _P, _P, _P, -1, 0, *_SC, None) == -1
    assert lib.pt_adamw_step(_P, _P, _P, _P, 8, 2, *_SC, None) == -1
    assert lib.pt_adamw_step(_P, _P, _P, _P, 0, 0, *_SC, None) == 0
    assert lib.pt_adamw_step(_P, _P, _P, _P, 0, 1, *_SC, None) == 0
    assert lib.pt_adamw_step(_P, _P, _P, _P, 0, 2, *_SC, None) == -1
    # list form: table, chunk_start, ntensors, total_chunks
    assert lib.pt_adamw_step_multi(None, _P, 1, 1, *_SC, None) == -1
    assert lib.pt_adamw_step_multi(_P, None, 1, 1, *_SC, None) == -1
    assert lib.pt_adamw_step_multi(_P, _P, 0, 1, *_SC, None) == -1
    assert lib.pt_adamw_step_multi(_P, _P, 1, -1, *_SC, None) == -1
    assert lib.pt_adamw_step_multi(_P, _P, 1, 0, *_SC, None) == 0


def _single_cases(nptr, dtype):
    """(arguments in front of the scalars, expected return) of a single-tensor step entry."""
    ok = (_P,) * nptr
    cases = [(ok[:i] + (None,) + ok[i + 1:] + (8, dtype), -1) for i in range(nptr)]
    return cases + [(ok + (-1, dtype), -1), (ok + (8, 2), -1), (ok + (0, 2), -1), (ok + (8, -1), -1), (ok + (0, dtype), 0)]


def _list_cases(*dtype):
    """The same for a list entry (dtype: the master forms' gradient dtype argument)."""
    cases = [((None, _P, 1, 1) + dtype, -1), ((_P, None, 1, 1) + dtype, -1), ((_P, _P, 0, 1) + dtype, -1),
             ((_P, _P, -1, 0) + dtype, -1), ((_P, _P, 1, -1) + dtype, -1), ((None, None, 1, 0) + dtype, -1),
             ((_P, _P, 1, 0) + dtype, 0)]
    if dtype:
        cases += [((_P, _P, 1, 1, 2), -1), ((_P, _P, 1, 0, 2), -1)]
    return cases


@pytest.mark.parametrize("name,cases", [
    ("pt_adamw_step", _single_cases(4, 0) + _single_cases(4, 1)),
    ("pt_adamw_step_multi", _list_cases()),
    ("pt_adamw_master_step_multi", _list_cases(0)),
    ("pt_adamw_master_step_multi", _list_cases(1)),
    ("pt_adamw_master_step", _single_cases(5, 0)),
    ("pt_adamw_master_step", _single_cases(5, 1)),
], ids=["step", "step_multi", "master_multi-bf16", "master_multi-f32", "master-bf16", "master-f32"])
def test_clipped_entries_refuse_what_their_namesakes_refuse(name, cases):
    """Every *_clip step entry, given valid clip arguments, returns what its unclipped namesake
    returns for the same leading arguments: the refusals (-1) and "nothing to do" (0).  And a
    clipped entry with a bad clip argument is refused even when there is nothing to do."""
    from picotron_amd import _C
    lib = _C.load_library()
    plain, clipped = getattr(lib, name), getattr(lib, name + "_clip")
    for lead, want in cases:
        assert plain(*lead, *_SC, None) == want, (name, lead)
        assert clipped(*lead, *_SC, _P, 1.0, None, None) == want, (name + "_clip", lead)
        for sq, max_norm in ((None, 1.0), (_P, 0.0), (_P, -1.0), (_P, float("nan"))):
            assert clipped(*lead, *_SC, sq, max_norm, None, None) == -1, (name + "_clip", lead, sq, max_norm)
