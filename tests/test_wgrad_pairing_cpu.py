"""Host logic of weight-gradient pairing (functional.WgradPairing / pair_jobs, train.train_step's
phases): which micro-batch defers its weight-gradient jobs, how the next one pairs them (kernels.KPair:
the two micro-batches' row blocks of one layout), and the phase sequence train_step drives.  The
K-segmented GEMM itself and the training numerics are GPU tests (test_kernels_gpu.py)."""
import torch

from picotron_amd import functional as FN
from picotron_amd import kernels as K


def _job(T, n, k, params):
    return (torch.randn(T, n), torch.randn(T, k), params)


def test_defer_then_pair():
    w1, w2 = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(6, 3))
    a, b = _job(8, 4, 3, [w1]), _job(8, 6, 3, [w2])
    old = FN.wgrad_pairing(0)
    try:
        assert FN.pair_jobs([a, b]) == [] and len(FN.WgradPairing.pending) == 2
        FN.wgrad_pairing(1)
        c, d = _job(8, 4, 3, [w1]), _job(8, 6, 3, [w2])
        out = FN.pair_jobs([c, d])
        assert not FN.WgradPairing.pending and len(out) == 2
        (dy, x, params), _ = out
        assert isinstance(dy, K.KPair) and dy.a is a[0] and dy.b is c[0] and x.a is a[1] and x.b is c[1]
        assert dy.shape == (16, 4) and params == [w1]
        sl = dy[:, 1:3]                                   # a column slice stays a pair
        assert isinstance(sl, K.KPair) and torch.equal(sl.a, a[0][:, 1:3]) and torch.equal(sl.b, c[0][:, 1:3])
        # a job of parameters nobody deferred passes through unpaired
        e = _job(8, 4, 3, [torch.nn.Parameter(torch.zeros(4, 3))])
        assert FN.pair_jobs([e]) == [e]
        FN.wgrad_pairing(None)
        assert FN.pair_jobs([e]) == [e]                   # phase None: as given
    finally:
        FN.wgrad_pairing(old)
        FN.WgradPairing.pending.clear()


def _recorded_launches(monkeypatch):
    """K.linear_wgrad / K.linear_wgrad_grouped replaced by recorders: [(dy2d, x2d, sinks, epilogue)]."""
    calls = []
    monkeypatch.setattr(K, "linear_wgrad", lambda dy, x, outs, epilogue=K.EPI_BF16, tile=-1:
                        calls.append((dy, x, outs, epilogue)))
    monkeypatch.setattr(K, "linear_wgrad_grouped", lambda jobs, epilogue=K.EPI_BF16, tile=-1:
                        calls.extend((dy, x, outs, epilogue) for dy, x, outs in jobs))
    return calls


def _deferred_twice(monkeypatch, defer):
    """Two jobs of one parameter deferred (phase 0) with no completing micro-batch between them, then
    the flush: BOTH reach the sink, the older first (on its own, when the newer takes its place)."""
    calls = _recorded_launches(monkeypatch)
    w = torch.nn.Parameter(torch.zeros(4, 3))
    a, b = _job(8, 4, 3, [w]), _job(8, 4, 3, [w])
    old = FN.wgrad_pairing(0)
    try:
        defer(a, b)
        assert [c[0] for c in calls] == [a[0]] and list(FN.WgradPairing.pending.values()) == [b]
        FN.wgrad_pairing(None)
        FN.flush_wgrad_pairs()
        assert not FN.WgradPairing.pending
    finally:
        FN.wgrad_pairing(old)
        FN.WgradPairing.pending.clear()
    assert len(calls) == 2
    (dy0, x0, s0, e0), (dy1, x1, s1, e1) = calls
    assert dy0 is a[0] and x0 is a[1] and dy1 is b[0] and x1 is b[1]
    assert s0[0] is w.grad and s1[0] is w.grad and (e0, e1) == (K.EPI_BF16, K.EPI_BF16_ACC)


def test_key_deferred_twice_launches_the_older_job(monkeypatch):
    _deferred_twice(monkeypatch, lambda a, b: (FN.wgrad(*a), FN.wgrad(*b)))


def test_key_repeated_in_one_deferred_group(monkeypatch):
    _deferred_twice(monkeypatch, lambda a, b: FN.wgrad_group([a, b]))


def test_mixed_sinks_of_a_group_are_resolved_once(monkeypatch):
    """One .grad present, the others not: resolving a sink creates the missing .grad, so a second
    look would accumulate onto its uninitialised memory -- each parameter's first gradient is a store."""
    calls = _recorded_launches(monkeypatch)
    w1, w2, w3 = (torch.nn.Parameter(torch.zeros(4, 3)) for _ in range(3))
    w1.grad = torch.zeros(4, 3)
    a, b = _job(8, 8, 3, [w1, w2]), _job(8, 4, 3, [w3])
    FN.wgrad_group([a, b])
    assert [(c[2][0] is p.grad, c[3]) for c, p in zip(calls, (w1, w2, w3))] == \
        [(True, K.EPI_BF16_ACC), (True, K.EPI_BF16), (True, K.EPI_BF16)]
    assert torch.equal(calls[0][0], a[0][:, :4]) and torch.equal(calls[1][0], a[0][:, 4:]) and calls[2][0] is b[0]


def test_train_step_phase_sequence():
    """Micro-batches (0, 1), (2, 3), ... pair; an odd last micro-batch runs alone (phase None)."""
    from picotron_amd.train import pairing_phase

    def phases(ga):
        return [pairing_phase(i, ga) for i in range(ga)]
    assert phases(4) == [0, 1, 0, 1]
    assert phases(5) == [0, 1, 0, 1, None]
    assert phases(1) == [None]
    assert phases(32).count(1) == 16
