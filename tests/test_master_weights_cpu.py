"""The host side of optim.AdamW(master_weights=True, use_main_grad=True) and
DataParallelBucket.publish_grad, without a kernel: the state-dict policy, the batching of a step,
the constructor's argument checks, and the gradient the bucket wrapper leaves behind (2 gloo ranks)."""
import pytest
import torch
import torch.distributed as dist

from tests import _dist

BF16, F32 = torch.bfloat16, torch.float32


def _hand_state(params, master):
    """What two steps would have left, built by hand."""
    g = torch.Generator().manual_seed(1)
    state = {}
    for i, p in enumerate(params):
        dt = F32 if master and p.dtype == BF16 else p.dtype
        st = {"step": torch.tensor(2.0), "exp_avg": (torch.randn(p.shape, generator=g) * 0.01).to(dt),
              "exp_avg_sq": (torch.randn(p.shape, generator=g).abs() * 1e-4).to(dt)}
        if master and p.dtype == BF16:
            st["master_param"] = p.detach().float() + torch.randn(p.shape, generator=g) * 2.0 ** -12   # below a bf16 ulp
        state[i] = st
    return state


def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dt)) for s, dt in (((64,), BF16), ((5, 7), BF16), ((9,), F32))]


def test_load_state_dict_keeps_f32_state():
    from picotron_amd.optim import AdamW
    params = _params()
    opt = AdamW(params, lr=1e-3, master_weights=True)
    sd = {"state": _hand_state(params, True), "param_groups": opt.state_dict()["param_groups"]}
    opt.load_state_dict(sd)
    for i, p in enumerate(params):
        st, want = opt.state[p], sd["state"][i]
        assert st["step"].dtype == F32 and st["step"].item() == 2.0 and st["step"].device.type == "cpu"
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == F32 and torch.equal(st[k], want[k])
            assert p.dtype == F32 or st[k].data_ptr() != want[k].data_ptr()   # a copy, not the caller's tensor
        if p.dtype == BF16:
            assert st["master_param"].dtype == F32 and torch.equal(st["master_param"], want["master_param"])
            assert not torch.equal(st["master_param"], p.detach().float())   # (it did not go through bf16)
        else:
            assert "master_param" not in st
    # and out again: state_dict() carries the three tensors as they are
    out = opt.state_dict()["state"]
    assert out[0]["master_param"].dtype == F32 and torch.equal(out[0]["master_param"], sd["state"][0]["master_param"])


def test_load_state_dict_across_modes():
    from picotron_amd.optim import AdamW
    params = _params()
    master, plain = AdamW(params, master_weights=True), AdamW(params)
    groups = plain.state_dict()["param_groups"]
    bf16_state = {"state": _hand_state(params, False), "param_groups": groups}
    master.load_state_dict(bf16_state)
    for i, p in enumerate(params):
        st = master.state[p]
        assert "master_param" not in st   # taken from the parameter at the next step
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == F32 and torch.equal(st[k], bf16_state["state"][i][k].float())
    f32_state = {"state": _hand_state(params, True), "param_groups": groups}
    with pytest.raises(ValueError, match="master_weights=True"):
        plain.load_state_dict(f32_state)
    assert len(plain.state) == 0
    no_master = {"state": {i: {k: v for k, v in s.items() if k != "master_param"} for i, s in f32_state["state"].items()},
                 "param_groups": groups}
    with pytest.raises(ValueError, match="master_weights=True"):   # f32 moments alone are refused too
        plain.load_state_dict(no_master)
    plain.load_state_dict(bf16_state)   # its own kind still loads
    assert plain.state[params[0]]["exp_avg"].dtype == BF16


def _aligned(n, dtype, off=0):
    """n elements starting `off` elements past a 16-byte boundary"""
    size = torch.empty((), dtype=dtype).element_size()
    base = torch.zeros(n + 16 + off, dtype=dtype)
    skip = (-base.data_ptr() % 16) // size + off
    v = base[skip:skip + n]
    assert v.data_ptr() % 16 == (off * size) % 16
    return v


def test_batches_group_by_step_listable_and_grad_dtype():
    from picotron_amd import optim
    shapes = [64, 24, 40, 16, 32, 8]
    ps = [torch.nn.Parameter(_aligned(n, BF16)) for n in shapes[:5]]
    ps.append(torch.nn.Parameter(_aligned(8, BF16, off=1)))     # an unaligned view
    pf = torch.nn.Parameter(_aligned(12, F32))                  # an f32 parameter: no master
    opt = optim.AdamW(ps + [pf], lr=1e-3, master_weights=True, use_main_grad=True)
    for p in ps[:2] + [ps[5], pf]:
        p.grad = _aligned(p.numel(), p.dtype)
    ps[2].main_grad = _aligned(40, F32)
    ps[3].main_grad = _aligned(16, F32)
    ps[3].grad = _aligned(16, BF16)                             # ignored: main_grad wins
    ps[4].main_grad = _aligned(32, BF16)                        # a bf16 main_grad joins the bf16 list
    got = {}
    for sc, kind, items in opt._batches(opt.param_groups[0]):
        dt = items[0][2].dtype if kind.startswith("master") else None
        assert (kind, dt) not in got
        got[(kind, dt)] = items
        assert sc["bc2_sqrt"] == (1 - 0.999 ** 1.0) ** 0.5
    assert sorted(got, key=str) == sorted([(optim.MASTER_MULTI, BF16), (optim.MASTER_MULTI, F32),
                                           (optim.MASTER_SINGLE, BF16), (optim.SINGLE, None)], key=str)
    assert [it[1] is p for it, p in zip(got[(optim.MASTER_MULTI, BF16)], (ps[0], ps[1], ps[4]))] == [True] * 3
    assert [it[1] is p for it, p in zip(got[(optim.MASTER_MULTI, F32)], (ps[2], ps[3]))] == [True] * 2
    assert got[(optim.MASTER_MULTI, F32)][1][2] is ps[3].main_grad
    (single,) = got[(optim.MASTER_SINGLE, BF16)]
    assert single[1] is ps[5] and single[1].data_ptr() % 16 == 2
    ((p, g, m, v),) = got[(optim.SINGLE, None)]
    assert p is pf and m.dtype == F32 and "master_param" not in opt.state[pf]
    for p in ps:
        st = opt.state[p]
        assert st["master_param"].dtype == st["exp_avg"].dtype == st["exp_avg_sq"].dtype == F32
        assert torch.equal(st["master_param"], p.detach().float()) and st["step"].item() == 1.0
    # a parameter one step behind the others (its gradient was None so far) gets a batch of its own
    late = torch.nn.Parameter(_aligned(16, BF16))
    opt.add_param_group(dict(params=[late]))
    late.grad = _aligned(16, BF16)
    steps = sorted((sc["bc2_sqrt"], kind, len(items)) for grp in opt.param_groups for sc, kind, items in opt._batches(grp)
                   if kind == optim.MASTER_MULTI and items[0][2].dtype == BF16)
    assert [(k, n) for _, k, n in steps] == [(optim.MASTER_MULTI, 1), (optim.MASTER_MULTI, 3)]
    assert steps[0][0] == (1 - 0.999 ** 1.0) ** 0.5 and steps[1][0] == (1 - 0.999 ** 2.0) ** 0.5
    # the default optimizer batches as before: bf16 list / the rest, no master state
    plain = optim.AdamW(ps[:2] + [ps[5], pf], lr=1e-3)
    kinds = sorted((kind, len(items)) for _, kind, items in plain._batches(plain.param_groups[0]))
    assert kinds == [(optim.MULTI, 2), (optim.SINGLE, 2)]
    assert all("master_param" not in plain.state[p] and plain.state[p]["exp_avg"].dtype == p.dtype for p in plain.state)


def test_constructor_validation():
    from picotron_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(8, dtype=BF16))]
    with pytest.raises(ValueError, match="master_weights"):
        AdamW(p, use_main_grad=True)
    with pytest.raises(ValueError):
        AdamW(p, master_weights=True, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        AdamW(p, master_weights=True, amsgrad=True)
    a = AdamW(p)
    assert (a.master_weights, a.use_main_grad, a.max_grad_norm) == (False, False, None)
    b = AdamW(p, master_weights=True)
    assert (b.master_weights, b.use_main_grad) == (True, False)
    c = AdamW(p, master_weights=True, use_main_grad=True, max_grad_norm=1.0)
    assert (c.master_weights, c.use_main_grad, c.max_grad_norm) == (True, True, 1.0)
    c.sync_master_from_params()   # nothing to do before the first step


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """PT_EINVAL (-1) from the host-side checks: no device is touched (there is none here)."""
    from picotron_amd import _C
    lib = _C.load_library()
    sc = (0.999, 0.1, 0.999, 0.001, 0.03, 1e-8, -3e-4)
    one = 16   # any non-null address: the checks return before it is read
    assert lib.pt_adamw_master_step_multi(None, None, 1, 1, 0, *sc, None) == -1
    assert lib.pt_adamw_master_step_multi(one, one, 0, 1, 0, *sc, None) == -1
    assert lib.pt_adamw_master_step_multi(one, one, 1, 1, 2, *sc, None) == -1          # grad dtype
    assert lib.pt_adamw_master_step_multi(one, one, 1, 0, 1, *sc, None) == 0           # nothing to do
    assert lib.pt_adamw_master_step_multi_clip(one, one, 1, 1, 0, *sc, None, 1.0, None, None) == -1
    assert lib.pt_adamw_master_step_multi_clip(one, one, 1, 1, 0, *sc, one, 0.0, None, None) == -1
    assert lib.pt_adamw_master_step(None, one, one, one, one, 8, 0, *sc, None) == -1
    assert lib.pt_adamw_master_step(one, one, one, one, one, -1, 0, *sc, None) == -1
    assert lib.pt_adamw_master_step(one, one, one, one, one, 8, 3, *sc, None) == -1
    assert lib.pt_adamw_master_step(one, one, one, one, one, 0, 1, *sc, None) == 0
    assert lib.pt_adamw_master_step_clip(one, one, one, one, one, 8, 0, *sc, None, 1.0, None, None) == -1
    assert lib.pt_adamw_master_step_clip(one, one, one, one, one, 8, 0, *sc, one, -1.0, None, None) == -1
    assert lib.pt_grad_sq_master_multi(one, one, 1, 1, 0, 1.0, 0, None, one, None) == -1
    assert lib.pt_grad_sq_master_multi(one, one, 1, 1, 5, 1.0, 0, one, one, None) == -1


def _dp_publish(rank, world, publish):
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.data_parallel.data_parallel import DataParallelBucket
    from tests.test_parallel_cpu import _Net
    pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=world)
    model = DataParallelBucket(_Net())
    assert model.publish_grad is True
    model.publish_grad = publish
    ref = _Net()
    ga = 2
    grads = {n: torch.zeros_like(p) for n, p in ref.named_parameters()}
    for i in range(ga):
        g = torch.Generator().manual_seed(100 * i + rank)
        ids = torch.randint(0, 16, (5,), generator=g)
        model.require_backward_grad_sync = (i == ga - 1)
        (model(ids).square().mean() / ga).backward()
        ref.zero_grad()
        (ref(ids).square().mean() / ga).backward()
        for n, p in ref.named_parameters():
            grads[n] += p.grad
    for n, p in model.module.named_parameters():
        want = grads[n].clone()
        dist.all_reduce(want)
        want /= world
        assert p.main_grad.dtype == torch.float32
        torch.testing.assert_close(p.main_grad, want, rtol=1e-5, atol=1e-6)
        if publish:
            assert torch.equal(p.grad, p.main_grad.to(p.dtype))
        else:
            assert p.grad is None
    model.reset()
    for p in model.module.parameters():
        assert p.main_grad.abs().sum().item() == 0.0


@pytest.mark.parametrize("publish", [False, True])
def test_dp_bucket_publish_grad(publish):
    _dist.run(_dp_publish, 2, publish)
