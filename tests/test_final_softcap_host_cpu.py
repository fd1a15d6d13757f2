"""Host side of the final-logit soft-capping entries (CPU): the codes of include/picotron_hip.h's section -- a refused
call launches nothing, so the fake pointers are never read -- and the wrappers' keyword check."""
import pytest

PTR = 1 << 20   # a non-null, 16-byte aligned address no refused call dereferences
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


def call(lib, entry, first=PTR, softcap=30.0, cols=64):   # `entry` with its first pointer at `first`, the rest regular
    args = {"pt_softcap_fwd": (cols, PTR, cols, 8, cols),
            "pt_softcap_bwd": (cols, PTR, cols, PTR, cols, 8, cols),
            "pt_gemm_ce_stats_cap": (64, PTR, 64, PTR, 512, PTR, 256, 256, 512, cols),
            "pt_cross_entropy_bwd_lse_cap": (cols, PTR, PTR, PTR, cols, 8, cols, PTR, 0, -100, 0.0),
            "pt_cross_entropy_fwd_bwd_cap": (cols, PTR, PTR, cols, PTR, 8, cols, 1.0, None, -100, None, 0.0, None)}[entry]
    return getattr(lib, entry)(first, *args, softcap, None)


ENTRIES = ["pt_softcap_fwd", "pt_softcap_bwd", "pt_gemm_ce_stats_cap", "pt_cross_entropy_bwd_lse_cap",
           "pt_cross_entropy_fwd_bwd_cap"]
CASES = [
    (dict(first=None), EINVAL), (dict(softcap=0.0), EINVAL), (dict(softcap=-2.0), EINVAL),
    (dict(softcap=float("inf")), EINVAL), (dict(softcap=float("nan")), EINVAL),
    (dict(cols=60), {"pt_gemm_ce_stats_cap": EUNSUPPORTED}),   # the namesake's own check: K % 64 / cols % 8
    (dict(softcap=0.0, cols=60), EINVAL),                      # precedence: the cap before the shape
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("args,code", CASES, ids=[",".join(f"{k}={v}" for k, v in c[0].items()) for c in CASES])
def test_entries_refuse_before_launch(entry, args, code):
    from picotron_amd import _C
    code = code.get(entry, EALIGN) if isinstance(code, dict) else code
    assert call(_C.load_library(), entry, **args) == code


def test_dropped_capped_forward_leaves_nothing(monkeypatch):
    import gc
    import weakref
    import torch   # (the table beside the logits holds the raw stand-in, and so the graph, weakly)
    from picotron_amd import functional as FN, kernels as K
    monkeypatch.setattr(K, "linear_fwd", lambda x, ws: x @ ws[0].T)
    monkeypatch.setattr(K, "softcap_fwd_", lambda y, c: y)
    FN._CE_STATS.clear()
    refs = []
    for _ in range(3):
        x, w = (torch.randn(n, 8, dtype=torch.bfloat16, requires_grad=True) for n in (4, 16))
        t = FN.as_logits(FN.lm_head_linear(x, w, softcap=30.0)).view(-1, 16)   # the first two holders are dropped
        assert FN._peek_cap(FN._plain(t)).raw() is not None
        refs.append(weakref.ref(x))
        del x, w, t
    gc.collect()
    assert all(e[0]() is None for e in FN._CE_STATS.values()) and all(r() is None for r in refs)


@pytest.mark.parametrize("bad", [-1.0, float("inf"), float("nan"), "30", True])
def test_keyword_refused_before_the_library(monkeypatch, bad):
    from picotron_amd import _C, kernels as K
    monkeypatch.setattr(_C, "lib", lambda: pytest.fail("the library was touched"))
    for f in (lambda: K.linear_ce_stats(None, None, softcap=bad), lambda: K.softcap_fwd_(None, bad),
              lambda: K.softcap_bwd_(None, None, bad), lambda: K.cross_entropy_grad_lse(None, None, None, None, softcap=bad),
              lambda: K.cross_entropy_fwd_bwd(None, None, softcap=bad)):
        with pytest.raises(ValueError, match="softcap"):
            f()
    assert K.softcap_coef(None) is None and K.softcap_coef(0) is None and K.softcap_coef(30) == 30.0
