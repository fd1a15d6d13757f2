"""The native host code of csrc/gemm.hip, pinned without a GPU.

The real library loads on a machine with no device, and its argument checks return before any HIP
call.  Two tables are replayed against tests/golden/gemm_host.json and compared exactly:

  * pt_gemm_pick_tile: the tile the auto-pick chooses over a grid of unsegmented [M, N] problems
    (PICK_SIZES squared), for a few problems with segment boundaries on and off the 64 / 128 / 256
    grids, and for a problem no tile divides (PICK_SEGMENTED);
  * refusals: for each of the seven launching pt_gemm* entry points, calls that must be refused,
    with the return code (REFUSALS).  Pointers are fake, non-null, 16-byte-aligned integers: they
    are never dereferenced because the call refuses.  Every row holds at least one violation; the
    rows marked (2) hold two and pin which check answers first.

`python tests/test_gemm_host_cpu.py` writes the golden file.  It was generated once, from the
commit before the host code was refactored, and is never regenerated to make a refactor pass: a
refactor of the host code keeps every code in it.  The generator asserts that every recorded
refusal is negative -- a call the library accepts has no place in the table (it would launch a
kernel on fake pointers).

The comment beside each row names the `return PT_E...` statement of that commit's host code it
reaches, by function and condition.  Statements of that commit with no row, because no call through
the ABI reaches them:

  * fill_split's `a.bseg[i] % BK` (split-K over K-segments): fill_args has refused the same
    boundaries before fill_split runs;
  * launch_layout's `default` of the general layouts (a retired or unknown tile id): args_fit has
    refused the id before any layout is looked at (the rows tile4 .. tile99 end there);
  * launch_mix_rope's PT_EUNSUPPORTED is no refusal: the caller goes on to launch one tile shape."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_host.json")

PICK_SIZES = (64, 128, 192, 256, 384, 512, 768, 1024, 2048, 4096, 49152)
# (M, N, M boundaries or None, N boundaries or None)
PICK_SEGMENTED = [
    (768, 4096, [0, 256, 512, 768], None),       # row segments on the 256 grid
    (768, 4096, [0, 128, 768], None),            # on the 128 grid only
    (768, 4096, [0, 64, 768], None),             # on the 64 grid only
    (768, 4096, [0, 96, 768], None),             # on none
    (4096, 768, None, [0, 256, 512, 768]),       # column segments on the 256 grid
    (4096, 768, None, [0, 128, 768]),            # on the 128 grid only
    (4096, 768, None, [0, 64, 768]),             # on the 64 grid only
    (4096, 768, None, [0, 100, 768]),            # on none
    (2048, 6144, None, [0, 2048, 4096, 6144]),   # the q|k|v projection
    (512, 1024, [0, 256, 512], [0, 128, 1024]),  # both: 256 rows, 128 columns
    (100, 100, None, None),                      # no tile divides it: -1
]

EPI_BF16, EPI_BF16_ACC, EPI_F32, EPI_F32_ACC, EPI_BF16_RES, EPI_SWIGLU_FWD, EPI_SWIGLU_BWD, EPI_ROPE, EPI_CE_STATS = \
    range(9)

A, A2, R, COS, SIN, STATS, PARTS, P1, OUT = (0x10000000 + i * 0x100000 for i in range(9))
B = [0x20000000 + i * 0x100000 for i in range(4)]
C = [0x30000000 + i * 0x100000 for i in range(4)]


def problem(**over):
    """One [256, 256] x K 256 problem with unsegmented operands (every leading dimension 256)."""
    p = dict(A=A, lda=256, B=[B[0]], ldb=[256], b_bounds=None, nb=1, b_seg_dim=0, C=[C[0]], ldc=[256], c_bounds=None,
             nc=1, M=256, N=256, K=256, residual=None, ldr=0, ksplit=0, kpart_stride=0, A2=None, a_k2=0)
    unknown = set(over) - set(p)
    assert not unknown, unknown
    p.update(over)
    return p


# the gate|up projection with SwiGLU: B = {W_gate, W_up}, C = {h [M, N / 2], g|u [M, N]}
SF = dict(epilogue=EPI_SWIGLU_FWD, N=512, nb=2, B=B[:2], ldb=[256, 256], nc=2, C=C[:2], ldc=[256, 512])
# dh = dY . W_down with the SwiGLU backward: R = g|u [M, 2N], C = dg|du [M, 2N]
SB = dict(epilogue=EPI_SWIGLU_BWD, b_kcontig=0, residual=R, ldr=512, ldc=[512])
RES = dict(epilogue=EPI_BF16_RES, residual=R, ldr=256)
KSEG = dict(b_seg_dim=1, nb=2, B=B[:2], ldb=[256, 256], b_bounds=[0, 128, 256])
NSEG = dict(N=512, nb=2, B=B[:2], ldb=[256, 256], b_bounds=[0, 128, 512], ldc=[512])
MSEG = dict(M=512, nc=2, C=C[:2], ldc=[256, 256], c_bounds=[0, 128, 512])
SPLIT = dict(ksplit=2, kpart_stride=65536)
SEG_A = dict(A2=A2, a_k2=128)

DEFAULTS = {
    "pt_gemm": dict(a_kcontig=1, b_kcontig=1, epilogue=EPI_BF16, tile=-1),
    "pt_gemm_grouped": dict(probs=[{}], nprob=None, a_kcontig=1, b_kcontig=1, epilogue=EPI_BF16, tile=-1),
    # group 0 = dX (A K-contiguous, B N-contiguous), group 1 = wgrad (both MN-contiguous)
    "pt_gemm_dual": dict(p0=[{}], n0=None, a_kcontig0=1, b_kcontig0=0, epilogue0=EPI_BF16, p1=[{}], n1=None,
                         a_kcontig1=0, b_kcontig1=0, epilogue1=EPI_BF16, order=0),
    "pt_gemm_rope": dict(cos=COS, sin=SIN, table_stride=64, seq_len=128, rot_cols=128, head_dim=64, tile=-1),
    "pt_gemm_ce_stats": dict(stats=STATS, block=256),
    "pt_gemm_splitk_reduce": dict(parts=PARTS, nparts=2, part_stride=65536, M=256, N=256, C=[C[0]], ldc=[256],
                                  c_bounds=None, nc=1, mode=EPI_BF16, residual=None, ldr=0),
    "pt_gemm_splitk_sum": dict(p0=PARTS, p1=P1, residual=None, out=OUT, n=1024),
}
PROBLEM_ENTRIES = ("pt_gemm", "pt_gemm_rope", "pt_gemm_ce_stats")   # take one problem's fields as arguments

G, GG, GD, GR, GC, SR, SS = DEFAULTS
# (entry point, case name, overrides of the entry's defaults)   # the statement reached
REFUSALS = [
    (G, "null_A", dict(A=None)),                                           # fill_args: null / counts / sizes
    (G, "null_B", dict(B=None)),                                           # fill_args: null / counts / sizes
    (G, "null_C", dict(C=None)),                                           # fill_args: null / counts / sizes
    (G, "nb0", dict(nb=0)),                                                # fill_args: null / counts / sizes
    (G, "nb5", dict(nb=5)),                                                # fill_args: null / counts / sizes
    (G, "nc0", dict(nc=0)),                                                # fill_args: null / counts / sizes
    (G, "nc5", dict(nc=5)),                                                # fill_args: null / counts / sizes
    (G, "M0", dict(M=0)),                                                  # fill_args: null / counts / sizes
    (G, "N0", dict(N=0)),                                                  # fill_args: null / counts / sizes
    (G, "K_negative", dict(K=-64)),                                        # fill_args: null / counts / sizes
    (G, "null_A+K_mod", dict(A=None, K=96)),                               # fill_args: null / counts / sizes (2)
    (G, "res_no_residual", dict(RES, residual=None)),                      # fill_args: EPI_BF16_RES residual
    (G, "res_nc2", dict(RES, **MSEG)),                                     # fill_args: EPI_BF16_RES residual
    (G, "res_unaligned", dict(RES, residual=R + 8)),                       # fill_args: EPI_BF16_RES residual
    (G, "res_ldr", dict(RES, ldr=260)),                                    # fill_args: EPI_BF16_RES residual
    (G, "res_no_residual+K_mod", dict(RES, residual=None, K=96)),          # fill_args: EPI_BF16_RES residual (2)
    (G, "sf_nb1", dict(SF, nb=1)),                                         # fill_args: EPI_SWIGLU_FWD operands
    (G, "sf_bdim1", dict(SF, b_seg_dim=1)),                                # fill_args: EPI_SWIGLU_FWD operands
    (G, "sf_nc1", dict(SF, nc=1)),                                         # fill_args: EPI_SWIGLU_FWD operands
    (G, "sf_N_odd", dict(SF, N=511)),                                      # fill_args: EPI_SWIGLU_FWD operands
    (G, "sf_ldb_differ", dict(SF, ldb=[256, 264])),                        # fill_args: EPI_SWIGLU_FWD operands
    (G, "sf_nb1+A_unaligned", dict(SF, nb=1, A=A + 8)),                    # fill_args: EPI_SWIGLU_FWD operands (2)
    (G, "sf_bounds", dict(SF, b_bounds=[0, 128, 512])),                    # fill_args: EPI_SWIGLU_FWD b_bounds
    (G, "sf_bounds_first", dict(SF, b_bounds=[64, 256, 512])),             # fill_args: EPI_SWIGLU_FWD b_bounds
    (G, "sf_bounds+B_unaligned", dict(SF, b_bounds=[0, 128, 512], B=[B[0] + 8, B[1]])),  # fill_args: EPI_SWIGLU_FWD b_bounds (2)
    (G, "sf_B1_unaligned", dict(SF, B=[B[0], B[1] + 8])),                  # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_B0_null", dict(SF, B=[None, B[1]])),                           # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_ldb_mod", dict(SF, ldb=[260, 260])),                           # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_C1_null", dict(SF, C=[C[0], None])),                           # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_C0_unaligned", dict(SF, C=[C[0] + 2, C[1]])),                  # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_ldc_mod", dict(SF, ldc=[256, 516])),                           # fill_args: EPI_SWIGLU_FWD B / C alignment
    (G, "sf_A_unaligned", dict(SF, A=A + 8)),                              # fill_args: EPI_SWIGLU_FWD A / K
    (G, "sf_lda_mod", dict(SF, lda=260)),                                  # fill_args: EPI_SWIGLU_FWD A / K
    (G, "sf_K_mod", dict(SF, K=96)),                                       # fill_args: EPI_SWIGLU_FWD A / K
    (G, "sf_tile13", dict(SF, tile=13)),                                   # launch_swiglu: tile
    (G, "sf_tile2", dict(SF, tile=2)),                                     # launch_swiglu: tile
    (G, "sf_M_mod", dict(SF, M=128)),                                      # launch_swiglu: M % 256 / N % tile
    (G, "sf_N_mod", dict(SF, N=384)),                                      # launch_swiglu: M % 256 / N % tile
    (G, "sf_a_mcontig", dict(SF, a_kcontig=0)),                            # launch_swiglu: EPI_SWIGLU_FWD layout
    (G, "sf_b_ncontig", dict(SF, b_kcontig=0)),                            # launch_swiglu: EPI_SWIGLU_FWD layout
    (G, "sb_no_residual", dict(SB, residual=None)),                        # fill_args: EPI_SWIGLU_BWD residual
    (G, "sb_nc2", dict(SB, **dict(MSEG, ldc=[512, 512]))),                 # fill_args: EPI_SWIGLU_BWD residual
    (G, "sb_res_unaligned", dict(SB, residual=R + 8)),                     # fill_args: EPI_SWIGLU_BWD residual
    (G, "sb_ldr_mod", dict(SB, ldr=516)),                                  # fill_args: EPI_SWIGLU_BWD residual
    (G, "sb_ldc_mod", dict(SB, ldc=[516])),                                # fill_args: EPI_SWIGLU_BWD residual
    (G, "sb_no_residual+K_mod", dict(SB, residual=None, K=96)),            # fill_args: EPI_SWIGLU_BWD residual (2)
    (G, "sb_tile13", dict(SB, tile=13)),                                   # launch_swiglu: tile
    (G, "sb_M_mod", dict(SB, M=128)),                                      # launch_swiglu: M % 256 / N % tile
    (G, "sb_N_mod", dict(SB, N=128)),                                      # launch_swiglu: M % 256 / N % tile
    (G, "sb_kseg", dict(SB, **KSEG)),                                      # launch_swiglu: EPI_SWIGLU_BWD segments
    (G, "sb_nseg", dict(SB, nb=2, B=B[:2], ldb=[256, 256], b_bounds=[0, 128, 256])),  # launch_swiglu: EPI_SWIGLU_BWD segments
    (G, "sb_a_mcontig", dict(SB, a_kcontig=0)),                            # launch_swiglu: EPI_SWIGLU_BWD layout
    (G, "sb_b_kcontig", dict(SB, b_kcontig=1)),                            # launch_swiglu: EPI_SWIGLU_BWD layout
    (G, "K_mod", dict(K=96)),                                              # fill_args: K % 64
    (G, "K_mod+B_unaligned", dict(K=96, B=[B[0] + 8])),                    # fill_args: K % 64 (2)
    (G, "M_big", dict(M=1 << 31)),                                         # fill_args: a size above INT32_MAX
    (G, "N_big+B_unaligned", dict(N=1 << 32, B=[B[0] + 8])),               # fill_args: a size above INT32_MAX (2)
    (G, "B_null_entry", dict(B=[None])),                                   # fill_args: B alignment
    (G, "B_unaligned", dict(B=[B[0] + 8])),                                # fill_args: B alignment
    (G, "ldb_mod", dict(ldb=[260])),                                       # fill_args: B alignment
    (G, "B_unaligned+b_bounds", dict(B=[B[0] + 8], b_bounds=[64, 256])),   # fill_args: B alignment (2)
    (G, "b_bounds_first", dict(b_bounds=[64, 256])),                       # fill_args: b_bounds ends
    (G, "b_bounds_last", dict(b_bounds=[0, 128])),                         # fill_args: b_bounds ends
    (G, "kseg_bounds_last", dict(KSEG, b_bounds=[0, 128, 512])),           # fill_args: b_bounds ends
    (G, "b_bounds_last+C_unaligned", dict(b_bounds=[0, 128], C=[C[0] + 8])),  # fill_args: b_bounds ends (2)
    (G, "C_null_entry", dict(C=[None])),                                   # fill_args: C alignment
    (G, "C_unaligned", dict(C=[C[0] + 8])),                                # fill_args: C alignment
    (G, "C_unaligned+c_bounds", dict(C=[C[0] + 8], c_bounds=[64, 256])),   # fill_args: C alignment (2)
    (G, "c_bounds_first", dict(c_bounds=[64, 256])),                       # fill_args: c_bounds ends
    (G, "c_bounds_last", dict(MSEG, c_bounds=[0, 128, 256])),              # fill_args: c_bounds ends
    (G, "c_bounds_first+A_unaligned", dict(c_bounds=[64, 256], A=A + 8)),  # fill_args: c_bounds ends (2)
    (G, "A_unaligned", dict(A=A + 8)),                                     # fill_args: A alignment
    (G, "lda_mod", dict(lda=260)),                                         # fill_args: A alignment
    (G, "A_unaligned+kseg_bounds_mod", dict(KSEG, A=A + 8, b_bounds=[0, 96, 256])),  # fill_args: A alignment (2)
    (G, "kseg_bounds_mod", dict(KSEG, b_bounds=[0, 96, 256])),             # fill_args: K-segment % 64
    (G, "kseg_bounds_mod+tile4", dict(KSEG, b_bounds=[0, 96, 256], tile=4)),  # fill_args: K-segment % 64 (2)
    (G, "rope_a_mcontig", dict(epilogue=EPI_ROPE, a_kcontig=0)),           # launch_group: EPI_ROPE layout
    (G, "rope_b_ncontig", dict(epilogue=EPI_ROPE, b_kcontig=0)),           # launch_group: EPI_ROPE layout
    (G, "rope_b_ncontig+tile2", dict(epilogue=EPI_ROPE, b_kcontig=0, tile=2)),  # launch_group: EPI_ROPE layout (2)
    (G, "no_tile_fits", dict(M=100, N=100, lda=256, ldc=[104])),           # launch_group: args_fit (auto pick: -1)
    (G, "tile4", dict(tile=4)),                                            # launch_group: args_fit (retired id)
    (G, "tile5", dict(tile=5)),                                            # launch_group: args_fit (retired id)
    (G, "tile8", dict(tile=8)),                                            # launch_group: args_fit (retired id)
    (G, "tile9", dict(tile=9)),                                            # launch_group: args_fit (retired id)
    (G, "tile0", dict(tile=0)),                                            # launch_group: args_fit (retired id)
    (G, "tile16", dict(tile=16)),                                          # launch_group: args_fit (id out of range)
    (G, "tile99", dict(tile=99)),                                          # launch_group: args_fit (id out of range)
    (G, "tile12_M_mod", dict(tile=12, M=128)),                             # launch_group: args_fit (M % BM)
    (G, "tile13_N_mod", dict(tile=13, N=192, ldc=[192])),                  # launch_group: args_fit (N % BN)
    (G, "tile15_M_mod", dict(tile=15, M=192)),                             # launch_group: args_fit (M % BM)
    (G, "tile12_cseg", dict(MSEG, tile=12)),                               # launch_group: args_fit (C segment % BM)
    (G, "tile12_nseg", dict(NSEG, tile=12)),                               # launch_group: args_fit (B N-segment % BN)
    (G, "tile14_nseg", dict(NSEG, b_bounds=[0, 64, 512], tile=14)),        # launch_group: args_fit (B N-segment % BN)
    (G, "tile12_kseg_ldb", dict(KSEG, ldb=[256, 264], tile=12)),           # launch_group: args_fit (phased: one ld over K-segments)
    (G, "tile15_kseg_ldb", dict(KSEG, ldb=[256, 264], tile=15)),           # launch_group: args_fit (phased: one ld over K-segments)
    (G, "epi9+no_tile_fits", dict(epilogue=9, M=100, N=100, ldc=[104])),   # launch_group: args_fit (2)
    (G, "a_mcontig_b_kcontig_tile12", dict(a_kcontig=0, tile=12)),         # launch_layout: !AK && BKC, a phased tile
    (G, "a_mcontig_b_kcontig_tile13", dict(a_kcontig=0, tile=13)),         # launch_layout: !AK && BKC, a phased tile
    (G, "a_mcontig_b_kcontig_tile14", dict(a_kcontig=0, tile=14)),         # launch_layout: !AK && BKC, a phased tile
    (G, "a_mcontig_b_kcontig_tile15", dict(a_kcontig=0, tile=15, epilogue=EPI_F32_ACC)),  # launch_layout: !AK && BKC, a phased tile
    (G, "res_b_ncontig", dict(RES, b_kcontig=0)),                          # launch_group: EPI_BF16_RES layout
    (G, "res_a_mcontig", dict(RES, a_kcontig=0, tile=2)),                  # launch_group: EPI_BF16_RES layout
    (G, "ce_a_mcontig", dict(epilogue=EPI_CE_STATS, a_kcontig=0, tile=12)),  # launch_group: EPI_CE_STATS layout
    (G, "ce_b_ncontig", dict(epilogue=EPI_CE_STATS, b_kcontig=0, tile=13)),  # launch_group: EPI_CE_STATS layout
    (G, "ce_tile14", dict(epilogue=EPI_CE_STATS, tile=14)),                # launch_group: EPI_CE_STATS tile
    (G, "ce_tile15", dict(epilogue=EPI_CE_STATS, tile=15)),                # launch_group: EPI_CE_STATS tile
    (G, "ce_tile2", dict(epilogue=EPI_CE_STATS, tile=2)),                  # launch_group: EPI_CE_STATS tile
    (G, "epi9", dict(epilogue=9)),                                         # launch_group: unknown epilogue
    (G, "epi_negative", dict(epilogue=-1, tile=12)),                       # launch_group: unknown epilogue

    (GG, "null_probs", dict(probs=None, nprob=1)),                         # pt_gemm_grouped: probs / nprob
    (GG, "nprob0", dict(nprob=0)),                                         # pt_gemm_grouped: probs / nprob
    (GG, "nprob5", dict(probs=[{}] * 5)),                                  # pt_gemm_grouped: probs / nprob
    (GG, "second_null_A", dict(probs=[{}, dict(A=None)])),                 # fill_args: null / counts / sizes
    (GG, "second_K_mod", dict(probs=[{}, dict(K=96)])),                    # fill_args: K % 64
    (GG, "a2_k0", dict(probs=[dict(SEG_A, a_k2=0)])),                      # fill_split: a_k2 range
    (GG, "a2_kK", dict(probs=[dict(SEG_A, a_k2=256)])),                    # fill_split: a_k2 range
    (GG, "a2_k_mod", dict(probs=[dict(SEG_A, a_k2=96)])),                  # fill_split: a_k2 range
    (GG, "a2_k0+a2_unaligned", dict(probs=[dict(A2=A2 + 8, a_k2=0)])),     # fill_split: a_k2 range (2)
    (GG, "a2_unaligned", dict(probs=[dict(SEG_A, A2=A2 + 8)])),            # fill_split: A2 alignment
    (GG, "a2_unaligned+split_epi", dict(probs=[dict(SEG_A, A2=A2 + 8, **SPLIT)])),  # fill_split: A2 alignment (2)
    (GG, "split_epi", dict(probs=[SPLIT])),                                # fill_split: split-K epilogue / stride / count
    (GG, "split_stride0", dict(probs=[dict(SPLIT, kpart_stride=0)], epilogue=EPI_F32)),  # fill_split: split-K epilogue / stride / count
    (GG, "split_65", dict(probs=[dict(SPLIT, ksplit=65)], epilogue=EPI_F32)),  # fill_split: split-K epilogue / stride / count
    (GG, "split_epi+split_K_mod", dict(probs=[dict(SPLIT, ksplit=3)])),    # fill_split: split-K epilogue / stride / count (2)
    (GG, "split_K_mod", dict(probs=[dict(SPLIT, ksplit=3)], epilogue=EPI_F32)),  # fill_split: K % (ksplit 64)
    (GG, "split_K_mod+tile4", dict(probs=[dict(SPLIT, ksplit=8)], epilogue=EPI_F32, tile=4)),  # fill_split: K % (ksplit 64) (2)
    (GG, "a2_tile13", dict(probs=[SEG_A], tile=13)),                       # launch_group: A2 with a tile other than 12
    (GG, "a2_tile2", dict(probs=[SEG_A], tile=2)),                         # launch_group: A2 with a tile other than 12
    (GG, "a2_tile15", dict(probs=[SEG_A], tile=15)),                       # launch_group: A2 with a tile other than 12
    (GG, "a2_auto_small", dict(probs=[SEG_A])),                            # launch_group: A2 with a tile other than 12 (auto pick: 3)
    (GG, "second_M_mod_tile12", dict(probs=[{}, dict(M=128)], tile=12)),   # launch_group: args_fit (M % BM)
    (GG, "sb_second_kseg", dict(SB, probs=[{}, KSEG])),                    # launch_swiglu: EPI_SWIGLU_BWD segments

    (GD, "null_p0", dict(p0=None, n0=1)),                                  # pt_gemm_dual: groups / counts
    (GD, "null_p1", dict(p1=None, n1=1)),                                  # pt_gemm_dual: groups / counts
    (GD, "n0_0", dict(n0=0)),                                              # pt_gemm_dual: groups / counts
    (GD, "n1_5", dict(p1=[{}] * 5)),                                       # pt_gemm_dual: groups / counts
    (GD, "p1_null_A", dict(p1=[dict(A=None)])),                            # fill_args: null / counts / sizes
    (GD, "p0_split_epi", dict(p0=[SPLIT])),                                # fill_split: split-K epilogue / stride / count
    (GD, "p0_null_A+order3", dict(p0=[dict(A=None)], order=3)),            # fill_args: null / counts / sizes (2)
    (GD, "a0_mcontig", dict(a_kcontig0=0)),                                # launch_dual: layouts / order
    (GD, "b0_kcontig", dict(b_kcontig0=1)),                                # launch_dual: layouts / order
    (GD, "a1_kcontig", dict(a_kcontig1=1)),                                # launch_dual: layouts / order
    (GD, "b1_kcontig", dict(b_kcontig1=1)),                                # launch_dual: layouts / order
    (GD, "order3", dict(order=3)),                                         # launch_dual: layouts / order
    (GD, "order_negative", dict(order=-1)),                                # launch_dual: layouts / order
    (GD, "p0_M_mod", dict(p0=[dict(M=128)])),                              # launch_dual: group 0 args_fit(12)
    (GD, "p0_sb_nseg", dict(epilogue0=EPI_SWIGLU_BWD,
                            p0=[dict(residual=R, ldr=512, ldc=[512], nb=2, B=B[:2], ldb=[256, 256],
                                     b_bounds=[0, 256, 256])])),           # launch_dual: EPI_SWIGLU_BWD segments
    (GD, "p1_N_mod", dict(p1=[dict(N=128)])),                              # launch_dual: group 1 args_fit(12)
    (GD, "e0_acc", dict(epilogue0=EPI_BF16_ACC)),                          # launch_dual: group 0 epilogue
    (GD, "e0_f32_acc", dict(epilogue0=EPI_F32_ACC)),                       # launch_dual: group 0 epilogue
    (GD, "e1_res", dict(epilogue1=EPI_BF16_RES, p1=[dict(residual=R, ldr=256)])),  # launch_dual_e1: group 1 epilogue
    (GD, "e1_9", dict(epilogue1=9)),                                       # launch_dual_e1: group 1 epilogue
    (GD, "one_tile_each", dict()),                                         # launch_dual_t: t0 % 8 / t1 % 8
    (GD, "t1_one_tile", dict(p0=[dict(M=2048)])),                          # launch_dual_t: t0 % 8 / t1 % 8
    (GD, "t0_one_tile", dict(p1=[dict(N=2048, ldb=[2048], ldc=[2048])])),  # launch_dual_t: t0 % 8 / t1 % 8

    (GR, "null_cos", dict(cos=None)),                                      # pt_gemm_rope: tables / seq_len / rot_cols
    (GR, "null_sin", dict(sin=None)),                                      # pt_gemm_rope: tables / seq_len / rot_cols
    (GR, "seq0", dict(seq_len=0)),                                         # pt_gemm_rope: tables / seq_len / rot_cols
    (GR, "rot_negative", dict(rot_cols=-64)),                              # pt_gemm_rope: tables / seq_len / rot_cols
    (GR, "rot_above_N", dict(rot_cols=320)),                               # pt_gemm_rope: tables / seq_len / rot_cols
    (GR, "null_cos+head_dim128", dict(cos=None, head_dim=128)),            # pt_gemm_rope: tables / seq_len / rot_cols (2)
    (GR, "head_dim128", dict(head_dim=128)),                               # pt_gemm_rope: head_dim / rot_cols % 64
    (GR, "rot_mod", dict(rot_cols=96)),                                    # pt_gemm_rope: head_dim / rot_cols % 64
    (GR, "head_dim128+null_A", dict(head_dim=128, A=None)),                # pt_gemm_rope: head_dim / rot_cols % 64 (2)
    (GR, "null_A", dict(A=None)),                                          # fill_args: null / counts / sizes
    (GR, "K_mod", dict(K=96)),                                             # fill_args: K % 64
    (GR, "B_unaligned", dict(B=[B[0] + 8])),                               # fill_args: B alignment
    (GR, "auto_M_mod", dict(M=128)),                                       # launch_group: EPI_ROPE args_fit
    (GR, "tile12_M_mod", dict(M=128, tile=12)),                            # launch_group: EPI_ROPE args_fit
    (GR, "tile14_N_mod", dict(N=192, ldc=[192], tile=14)),                 # launch_group: EPI_ROPE args_fit
    (GR, "tile4", dict(tile=4)),                                           # launch_group: EPI_ROPE args_fit
    (GR, "tile15", dict(tile=15)),                                         # launch_group: EPI_ROPE tile
    (GR, "tile2", dict(tile=2)),                                           # launch_group: EPI_ROPE tile
    (GR, "tile3", dict(tile=3)),                                           # launch_group: EPI_ROPE tile

    (GC, "null_stats", dict(stats=None)),                                  # pt_gemm_ce_stats: stats
    (GC, "stats_unaligned", dict(stats=STATS + 8)),                        # pt_gemm_ce_stats: stats
    (GC, "null_stats+block64", dict(stats=None, block=64)),                # pt_gemm_ce_stats: stats (2)
    (GC, "block64", dict(block=64)),                                       # pt_gemm_ce_stats: block
    (GC, "block512", dict(block=512)),                                     # pt_gemm_ce_stats: block
    (GC, "block64+null_A", dict(block=64, A=None)),                        # pt_gemm_ce_stats: block (2)
    (GC, "null_A", dict(A=None)),                                          # fill_args: null / counts / sizes
    (GC, "W_unaligned", dict(B=[B[0] + 8])),                               # fill_args: B alignment
    (GC, "K_mod", dict(K=96)),                                             # fill_args: K % 64
    (GC, "K_mod+M_mod", dict(K=96, M=128)),                                # fill_args: K % 64 (2)
    (GC, "M_mod", dict(M=128)),                                            # pt_gemm_ce_stats: args_fit
    (GC, "block128_N_mod", dict(block=128, N=192, ldc=[192])),             # pt_gemm_ce_stats: args_fit
    (GC, "M_mod+ldc_mod", dict(M=128, ldc=[260])),                         # pt_gemm_ce_stats: args_fit (2)
    (GC, "ldc_mod", dict(ldc=[260])),                                      # pt_gemm_ce_stats: ldc % 8

    (SR, "null_parts", dict(parts=None)),                                  # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "nparts0", dict(nparts=0)),                                       # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "M0", dict(M=0)),                                                 # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "N_mod4", dict(N=258)),                                           # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "null_C", dict(C=None)),                                          # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "nc0", dict(nc=0)),                                               # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "nc5", dict(nc=5)),                                               # pt_gemm_splitk_reduce: null / counts / sizes
    (SR, "null_parts+stride_small", dict(parts=None, part_stride=1024)),   # pt_gemm_splitk_reduce: null / counts / sizes (2)
    (SR, "stride_small", dict(part_stride=1024)),                          # pt_gemm_splitk_reduce: parts / part_stride
    (SR, "parts_unaligned", dict(parts=PARTS + 8)),                        # pt_gemm_splitk_reduce: parts / part_stride
    (SR, "stride_mod", dict(part_stride=65538)),                           # pt_gemm_splitk_reduce: parts / part_stride
    (SR, "stride_small+res_missing", dict(part_stride=1024, mode=EPI_BF16_RES)),  # pt_gemm_splitk_reduce: parts / part_stride (2)
    (SR, "res_missing", dict(mode=EPI_BF16_RES)),                          # pt_gemm_splitk_reduce: residual
    (SR, "sb_res_unaligned", dict(mode=EPI_SWIGLU_BWD, residual=R + 4, ldr=512, ldc=[512])),  # pt_gemm_splitk_reduce: residual
    (SR, "res_ldr_mod", dict(mode=EPI_BF16_RES, residual=R, ldr=258)),     # pt_gemm_splitk_reduce: residual
    (SR, "res_missing+C_unaligned", dict(mode=EPI_BF16_RES, C=[C[0] + 4])),  # pt_gemm_splitk_reduce: residual (2)
    (SR, "sb_nc2", dict(mode=EPI_SWIGLU_BWD, residual=R, ldr=512, nc=2, C=C[:2], ldc=[512, 512],
                        c_bounds=[0, 128, 256])),                          # pt_gemm_splitk_reduce: EPI_SWIGLU_BWD nc
    (SR, "c_bounds_first", dict(c_bounds=[64, 256])),                      # pt_gemm_splitk_reduce: c_bounds ends
    (SR, "c_bounds_last", dict(nc=2, C=C[:2], ldc=[256, 256], c_bounds=[0, 128, 512])),  # pt_gemm_splitk_reduce: c_bounds ends
    (SR, "c_bounds_first+C_unaligned", dict(c_bounds=[64, 256], C=[C[0] + 4])),  # pt_gemm_splitk_reduce: c_bounds ends (2)
    (SR, "C_null_entry", dict(C=[None])),                                  # pt_gemm_splitk_reduce: C alignment
    (SR, "C_bf16_unaligned", dict(C=[C[0] + 4])),                          # pt_gemm_splitk_reduce: C alignment
    (SR, "C_f32_unaligned", dict(mode=EPI_F32, C=[C[0] + 8])),             # pt_gemm_splitk_reduce: C alignment
    (SR, "ldc_mod", dict(ldc=[258])),                                      # pt_gemm_splitk_reduce: C alignment
    (SR, "C_bf16_unaligned+mode9", dict(C=[C[0] + 4], mode=9)),            # pt_gemm_splitk_reduce: C alignment (2)
    (SR, "mode5", dict(mode=EPI_SWIGLU_FWD)),                              # pt_gemm_splitk_reduce: unknown mode
    (SR, "mode7", dict(mode=EPI_ROPE)),                                    # pt_gemm_splitk_reduce: unknown mode
    (SR, "mode9", dict(mode=9)),                                           # pt_gemm_splitk_reduce: unknown mode

    (SS, "null_p0", dict(p0=None)),                                        # pt_gemm_splitk_sum: null / n
    (SS, "null_p1", dict(p1=None)),                                        # pt_gemm_splitk_sum: null / n
    (SS, "null_out", dict(out=None)),                                      # pt_gemm_splitk_sum: null / n
    (SS, "n0", dict(n=0)),                                                 # pt_gemm_splitk_sum: null / n
    (SS, "n_mod4", dict(n=1026)),                                          # pt_gemm_splitk_sum: null / n
    (SS, "n_mod4+p0_unaligned", dict(n=1026, p0=PARTS + 8)),               # pt_gemm_splitk_sum: null / n (2)
    (SS, "p0_unaligned", dict(p0=PARTS + 8)),                              # pt_gemm_splitk_sum: alignment
    (SS, "p1_unaligned", dict(p1=P1 + 4)),                                 # pt_gemm_splitk_sum: alignment
    (SS, "out_unaligned", dict(out=OUT + 4)),                              # pt_gemm_splitk_sum: alignment
    (SS, "residual_unaligned", dict(residual=R + 4)),                      # pt_gemm_splitk_sum: alignment
]


# Refusals the host code gained after the golden file was written, pinned beside it in
# tests/golden/gemm_host_added.json (gemm_host.json is not regenerated; no code in it changed).
#   * K-segments of B with different leading dimensions on the simple tiles 2 / 3 (and the auto pick
#     that would land on them): every kernel steps a tile's B image with one leading dimension since
#     the segment bases moved into registers (BImg), but only the phased tiles refused such a call;
#     the simple kernels launched and read the later segments at the first one's stride, outside them.
#     Found by tests/test_gemm_conformance_gpu.py's K-segment test while reading bimg_ptr for bounds.
ADDED_GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_host_added.json")
ADDED_REFUSALS = [
    (G, "tile2_kseg_ldb", dict(KSEG, ldb=[256, 264], tile=2)),             # launch_group: args_fit (one ld over K-segments)
    (G, "tile3_kseg_ldb", dict(KSEG, ldb=[256, 264], tile=3)),             # launch_group: args_fit (one ld over K-segments)
    (G, "auto_kseg_ldb", dict(KSEG, ldb=[256, 264])),                      # launch_group: args_fit (auto pick: -1)
    (GG, "second_kseg_ldb_tile3", dict(probs=[{}, dict(KSEG, ldb=[256, 264])], tile=3)),  # launch_group: args_fit
]


def library():
    from picotron_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from picotron_amd import build
        build.build(verbose=False)
    return _C.load_library()


class variants_default:
    """The auto tile of a launch depends on the gemm_mix / gemm_kh variants: taken at their defaults."""
    VALUES = {b"gemm_mix": 1, b"gemm_kh": 2}

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = {n: self.lib.pt_get_variant(n) for n in self.VALUES}
        for n, v in self.VALUES.items():
            assert self.lib.pt_set_variant(n, v) == 0

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            self.lib.pt_set_variant(n, v)


def _ptrs(vals, keep):
    if vals is None:
        return None
    arr = (ctypes.c_void_p * len(vals))(*vals)
    keep.append(arr)
    return arr


def _i64s(vals, keep):
    from picotron_amd import _C
    if vals is None:
        return None
    arr = _C.i64arr(vals)
    keep.append(arr)
    return arr


def _struct(p):
    from picotron_amd import _C
    q = _C.GemmProblem()
    for name in ("A", "lda", "nb", "b_seg_dim", "nc", "M", "N", "K", "residual", "ldr", "ksplit", "kpart_stride", "A2",
                 "a_k2"):
        setattr(q, name, p[name])
    for name in ("B", "ldb", "C", "ldc"):
        for i, v in enumerate(p[name]):
            getattr(q, name)[i] = v if v is not None else 0
    # the struct always carries bounds: the unsegmented ones where the row gives none
    bb = p["b_bounds"] or [0] + [p["K"] if p["b_seg_dim"] else p["N"]] * p["nb"]
    cb = p["c_bounds"] or [0] + [p["M"]] * p["nc"]
    for i, v in enumerate(bb[:5]):
        q.b_bounds[i] = v
    for i, v in enumerate(cb[:5]):
        q.c_bounds[i] = v
    return q


def _group(probs, common, keep):
    from picotron_amd import _C
    if probs is None:
        return None
    arr = (_C.GemmProblem * max(len(probs), 1))(*[_struct(problem(**dict(common, **p))) for p in probs])
    keep.append(arr)
    return arr


def call(lib, entry, over, keep):
    a = dict(DEFAULTS[entry])
    if entry in PROBLEM_ENTRIES:
        a.update(problem())
    unknown = set(over) - set(a) - (set(problem()) if entry in (GG, GD) else set())
    assert not unknown, (entry, unknown)
    a.update(over)
    P, I = (lambda n: _ptrs(a[n], keep)), (lambda n: _i64s(a[n], keep))
    if entry == G:
        return lib.pt_gemm(a["A"], a["lda"], a["a_kcontig"], P("B"), I("ldb"), I("b_bounds"), a["nb"], a["b_kcontig"],
                           a["b_seg_dim"], P("C"), I("ldc"), I("c_bounds"), a["nc"], a["M"], a["N"], a["K"],
                           a["epilogue"], a["residual"], a["ldr"], a["tile"], None)
    if entry == GR:
        return lib.pt_gemm_rope(a["A"], a["lda"], P("B"), I("ldb"), I("b_bounds"), a["nb"], a["C"][0], a["ldc"][0],
                                a["M"], a["N"], a["K"], a["cos"], a["sin"], a["table_stride"], a["seq_len"],
                                a["rot_cols"], a["head_dim"], a["tile"], None)
    if entry == GC:
        return lib.pt_gemm_ce_stats(a["A"], a["lda"], a["B"][0], a["ldb"][0], a["C"][0], a["ldc"][0], a["stats"],
                                    a["block"], a["M"], a["N"], a["K"], None)
    if entry == GG:   # problem fields given beside `probs` apply to every problem of the group
        common = {k: v for k, v in a.items() if k in problem()}
        n = a["nprob"] if a["nprob"] is not None else len(a["probs"])
        return lib.pt_gemm_grouped(_group(a["probs"], common, keep), n, a["a_kcontig"], a["b_kcontig"], a["epilogue"],
                                   a["tile"], None)
    if entry == GD:
        n0 = a["n0"] if a["n0"] is not None else len(a["p0"])
        n1 = a["n1"] if a["n1"] is not None else len(a["p1"])
        return lib.pt_gemm_dual(_group(a["p0"], {}, keep), n0, a["a_kcontig0"], a["b_kcontig0"], a["epilogue0"],
                                _group(a["p1"], {}, keep), n1, a["a_kcontig1"], a["b_kcontig1"], a["epilogue1"],
                                a["order"], None)
    if entry == SR:
        return lib.pt_gemm_splitk_reduce(a["parts"], a["nparts"], a["part_stride"], a["M"], a["N"], P("C"), I("ldc"),
                                         I("c_bounds"), a["nc"], a["mode"], a["residual"], a["ldr"], None)
    assert entry == SS
    return lib.pt_gemm_splitk_sum(a["p0"], a["p1"], a["residual"], a["out"], a["n"], None)


def pick_rows(lib):
    from picotron_amd import _C
    rows = [[M, N, None, None, lib.pt_gemm_pick_tile(M, N, None, 0, None, 0)] for M in PICK_SIZES for N in PICK_SIZES]
    for M, N, ms, ns in PICK_SEGMENTED:
        rc = lib.pt_gemm_pick_tile(M, N, _C.i64arr(ms) if ms else None, len(ms or ()), _C.i64arr(ns) if ns else None,
                                   len(ns or ()))
        rows.append([M, N, ms, ns, rc])
    return rows


def refusal_codes(lib):
    out, keep = {}, []
    for entry, case, over in REFUSALS:
        key = f"{entry}/{case}"
        assert key not in out, key
        out[key] = call(lib, entry, over, keep)
    return out


def tables():
    lib = library()
    with variants_default(lib):
        return {"pick_tile": pick_rows(lib), "refusals": refusal_codes(lib)}


def test_rows_cover_every_entry_point_and_pin_check_order():
    assert {e for e, _, _ in REFUSALS} == set(DEFAULTS)
    assert sum(case.count("+") > 0 for _, case, _ in REFUSALS) >= 20
    # retired and out-of-range tile ids, A2 off tile 12, the !AK && BKC layout on a phased tile,
    # EPI_CE_STATS on tiles 14 / 15 and EPI_ROPE on tile 15
    cases = {f"{e}/{c}" for e, c, _ in REFUSALS}
    assert {f"{G}/tile{t}" for t in (4, 5, 8, 9, 16)} <= cases
    assert {f"{GG}/a2_tile13", f"{G}/a_mcontig_b_kcontig_tile12", f"{G}/ce_tile14", f"{G}/ce_tile15",
            f"{GR}/tile15"} <= cases


def test_pick_tile_matches_golden():
    want, got = json.load(open(GOLDEN))["pick_tile"], tables()["pick_tile"]
    assert len(got) == len(PICK_SIZES) ** 2 + len(PICK_SEGMENTED)
    assert got == want
    assert got[-1] == [100, 100, None, None, -1]
    assert {r[4] for r in got} >= {2, 3, 12, 13}


def test_refusals_match_golden():
    want, got = json.load(open(GOLDEN))["refusals"], tables()["refusals"]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(rc < 0 for rc in got.values())


def test_added_refusals_match_their_golden():
    lib = library()
    want = json.load(open(ADDED_GOLDEN))["refusals"]
    keep = []
    with variants_default(lib):
        got = {f"{e}/{c}": call(lib, e, over, keep) for e, c, over in ADDED_REFUSALS}
    assert got == want and all(rc < 0 for rc in got.values())
    assert not set(got) & set(json.load(open(GOLDEN))["refusals"])


if __name__ == "__main__":
    t = tables()
    accepted = {k: rc for k, rc in t["refusals"].items() if rc >= 0}
    assert not accepted, f"rows the library accepts have no place in the table: {accepted}"
    with open(GOLDEN, "w") as f:
        f.write('{\n "pick_tile": [\n' + ",\n".join("  " + json.dumps(r) for r in t["pick_tile"]) + "\n ],\n")
        f.write(' "refusals": {\n' + ",\n".join(f"  {json.dumps(k)}: {rc}" for k, rc in t["refusals"].items()))
        f.write("\n }\n}\n")
    print(f"wrote {GOLDEN}: {len(t['pick_tile'])} pick_tile rows, {len(t['refusals'])} refusals")
