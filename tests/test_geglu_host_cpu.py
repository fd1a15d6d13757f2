"""GeGLU host checks without a GPU (fake pointers as in tests/test_row_host_cpu.py: every call is refused before
a launch): pt_geglu_* answer as pt_swiglu_*; epilogues 10 / 11 are refused where 5 / 6 are; id 9 is unknown."""
import pytest

from tests import test_gemm_host_cpu as GH
from tests import test_row_host_cpu as RH

@pytest.mark.parametrize("over", [dict(g=None), dict(rows=0), dict(cols=60), dict(g_stride=68), dict(u=RH.P[1] + 8),
                                  dict(g=None, u=RH.P[1] + 8)])   # (the last: NULL and misaligned together)
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_row_entries_refuse_as_swiglu(direction, over):
    args = dict(RH.DEFAULTS["pt_swiglu_" + direction], **over)
    codes = [getattr(RH.library(), f"pt_{name}_{direction}")(*args.values(), None) for name in ("swiglu", "geglu")]
    assert codes[0] == codes[1] < 0


@pytest.mark.parametrize("entry,over", [   # refused with epilogue 5 / 6 and, but for nc = 2, not with an unknown id's code
    (GH.G, dict(GH.SF, N=384)), (GH.G, dict(GH.SF, tile=13)), (GH.G, dict(GH.SB, **dict(GH.MSEG, ldc=[512, 512]))),
    (GH.G, dict(GH.SB, b_kcontig=1)), (GH.GG, dict(GH.SB, probs=[{}, GH.KSEG]))])
def test_epilogues_10_11_refused_where_5_6_are(entry, over):
    lib, keep = GH.library(), []
    with GH.variants_default(lib):
        codes = [GH.call(lib, entry, o, keep) for o in (over, dict(over, epilogue=over["epilogue"] + 5))]
    assert codes[0] == codes[1] < 0
    assert GH.call(lib, GH.G, dict(epilogue=9), keep) == GH.call(lib, GH.SR, dict(mode=9), keep) == -1   # still unknown
