"""The tensor-parallel forms of the autograd layer (picotron_amd/functional.py) stage by stage on the GPU, on every rank:
the kernel calls AND the collectives of a forward + backward are recorded (tests/_tp_ref.py), every rank's roles
are exchanged, and each rank checks every stage of its own math per element from the production values of its
inputs -- the shard-local stages under the bounds of the kernels' own kits (tests/_model_ref.py), the gathered
buffers by bits against the documented token-row layout, every reduce-scatter / all-reduce output against the
float64 sum of the ranks' recorded partials, the norm weight gradients summed over the group, the vocab-parallel
entry, exit and cross-entropy -- and the issue / wait ledger.  No tolerance of this file's, no slack factor.

Each case is one spawn of W ranks that all drive cuda:0 and talk over gloo (tests/_dist.py).  Over gloo a
collective is complete when it returns: the ledger pins the HOST order of issue, consumers and wait in
_forward_sp / _backward_sp / attn_block_bwd / mlp_block_bwd, which would otherwise never run as asynchronous here.
A missing STREAM dependency under RCCL, with its asynchronous handles, is not visible on a one-GPU machine and is
not covered by this file.

Shapes: test_parallel_gpu.CFG's widths (H 256, I 512, heads 4 / 2 of 64, V 512) at B 2, S 128 -- T 256 rows, one
128-row attention block per sequence, with two chunks each chunk one sequence; at tp 2 the shards are 128 / 64 / 64
columns of q | k | v and 256 of gate, up and vocabulary.  loss / 4, ~5 % of the targets ignored, norm weights
away from 1.

    case        form
    sp_c2_L2    tp 2, tp_sp_chunks 2, 2 layers: the default chunked sequence-parallel layer, bf16 .grad sinks
                (chunk 0 stores, chunk 1 accumulates), the vocab-parallel CE
    sp_c1       tp 2, one chunk, 1 layer: every collective in one piece
    replicated  tp 2, tp_sp 0, vp_ce 0, 1 layer: the replicated stream, all-reduces, the gathered logits
    tp4         tp 4, 4 kv heads, 2 chunks, 1 layer: the W > 2 bounds, 32 rows per rank and chunk
    main_grad   tp 2 chunked, an f32 main_grad on every weight: f32 accumulate sinks across the chunks
    owner       tp 2 chunked, an owner waiting on the norm weights (_pt_grad_ready): the immediate
                _sp_sum_partials path and its notification

Worst |got - ref| / bound per role (rows) and case (columns) over the ranks, layers and chunks, measured on the MI355X
(test_zz_worst_ratio_table prints it; a bf16 store reaches its half ulp, so ratios near 1 are the bound at work;
0.000 is a comparison by bits; '-': the case has no such role).  Gathers: "h1 / h2 / dm / da / xf / dx0 gather";
sums: ar, mr, "dh2 sum", "dh1 sum" (the replicated form: out for mr), "dhf sum" (the lm_head dX), "x0 sum", dw1 / dw2 .sum (the
f32 block of _sp_sum_partials); dw1 / dw2 .dw: the layer norms' gradients summed over tp; "ce parts": max + log sum-exp
of the 16-byte parts (max, target logit and own are by bits inside it):

    role                                 sp_c2_L2      sp_c1 replicated        tp4  main_grad      owner
    a                                       0.980      0.980      0.980      0.991      0.980      0.980
    ar                                      0.000      0.000      0.000      0.664      0.000      0.000
    ce parts                                0.011      0.012          -      0.014      0.012      0.012
    ce_scale                                0.000      0.000      0.000      0.000      0.000      0.000
    dW_d                                    0.982      0.972      0.963      0.985      0.612      0.988
    dW_emb                                  0.000      0.000      0.000      0.000      0.000      0.000
    dW_g/dW_u.g                             0.984      0.976      0.966      0.978      0.735      0.979
    dW_g/dW_u.u                             0.986      0.957      0.970      0.974      0.735      0.981
    dW_lm                                   0.979      0.983      0.983      0.979      0.453      0.983
    dW_o                                    0.978      0.962      0.955      0.983      0.726      0.975
    dW_qkv.k                                0.978      0.948      0.948      0.986      0.852      0.981
    dW_qkv.q                                0.981      0.951      0.950      0.982      0.838      0.982
    dW_qkv.v                                0.984      0.954      0.952      0.978      0.710      0.977
    da gather                               0.000      0.000      0.000      0.000      0.000      0.000
    dgu.dg                                  0.996      0.996      0.996      0.995      0.996      0.996
    dgu.du                                  0.988      0.988      0.988      0.988      0.988      0.988
    dh1                                     0.958      0.976      0.961      0.963      0.976      0.976
    dh1 sum                                 0.000      0.000      0.000      0.664      0.000      0.000
    dh2                                     0.920      0.915      0.914      0.968      0.915      0.915
    dh2 sum                                 0.000      0.000      0.000      0.664      0.000      0.000
    dhf                                     0.986      0.982      0.986      0.991      0.982      0.982
    dhf sum                                 0.000      0.000      0.000      0.664      0.000      0.000
    dhh                                     0.949      0.954      0.945      0.953      0.954      0.954
    dlogits                                 0.995      0.995      0.995      0.994      0.995      0.995
    dm gather                               0.000      0.000      0.000      0.000      0.000      0.000
    do                                      0.942      0.963      0.935      0.942      0.963      0.963
    dout shard                              0.000      0.000      0.000      0.000      0.000      0.000
    dqkv_rot                                0.996      0.996      0.996      0.996      0.996      0.996
    dqkv_unrot.dk                           0.521      0.493      0.526      0.508      0.493      0.493
    dqkv_unrot.dq                           0.543      0.535      0.506      0.501      0.535      0.535
    dqkv_unrot.dv                           0.403      0.435      0.416      0.545      0.435      0.435
    dw1.dw                                  0.977      0.849          -      0.980      0.534      0.849
    dw1.sum                                 0.000      0.000          -      0.468      0.000      0.000
    dw2.dw                                  0.937      0.897          -      0.926      0.424      0.897
    dw2.sum                                 0.000      0.000          -      0.546      0.000      0.000
    dx.dw1                                      -          -      0.887          -          -          -
    dx.dx                                   0.996      0.991      0.995      0.995      0.991      0.991
    dx0 gather                              0.000      0.000      0.000      0.000      0.000      0.000
    dxf/dwf.dwf                             0.954      0.900      0.911      0.893      0.073      0.900
    dxf/dwf.dxf                             0.993      0.996      0.994      0.994      0.996      0.996
    dz.dw2                                      -          -      0.903          -          -          -
    dz.dz                                   0.996      0.995      0.995      0.996      0.995      0.995
    gu                                      0.949      0.945      0.945      0.962      0.945      0.945
    h1 gather                               0.000      0.000      0.000      0.000      0.000      0.000
    h1/rstd1.h1                             0.996      0.996      0.996      0.996      0.996      0.996
    h1/rstd1.rstd1                          0.118      0.109      0.109      0.109      0.109      0.109
    h2 gather                               0.000      0.000      0.000      0.000      0.000      0.000
    hf/rstdf.hf                             0.996      0.994      0.996      0.995      0.994      0.994
    hf/rstdf.rstdf                          0.150      0.141      0.130      0.127      0.141      0.141
    hh                                      0.988      0.988      0.988      0.988      0.988      0.988
    logits                                  0.947      0.946      0.939      0.943      0.946      0.946
    logits gather                               -          -      0.000          -          -          -
    loss.inv_count                          0.000      0.000      0.000      0.000      0.000      0.000
    loss.loss                               0.092      0.007      0.011      0.070      0.007      0.007
    m                                       0.963      0.970      0.976      0.985      0.970      0.970
    mr                                      0.000      0.000          -      0.664      0.000      0.000
    o/lse.lse                               0.047      0.044      0.044      0.044      0.044      0.044
    o/lse.o                                 0.460      0.419      0.419      0.436      0.419      0.419
    out                                     0.000      0.000      0.000      0.000      0.000      0.000
    qkv                                     0.996      0.996      0.996      0.996      0.996      0.996
    qkv_raw                                 0.947      0.948      0.948      0.948      0.948      0.948
    row_lse                                 0.051      0.048      0.077      0.050      0.048      0.048
    x0                                      0.000      0.000      0.000      0.000      0.000      0.000
    x0 sum                                  0.000      0.000      0.000      0.000      0.000      0.000
    x0 table                                0.000      0.000      0.000      0.000      0.000      0.000
    xf gather                               0.000      0.000      0.000      0.000      0.000      0.000
    z/h2/rstd2.h2                           0.993      0.996      0.996      0.996      0.996      0.996
    z/h2/rstd2.rstd2                        0.134      0.126      0.126      0.139      0.126      0.126
    z/h2/rstd2.z                            0.000      0.000      0.000      0.000      0.000      0.000

The sums over W = 4: over gloo functional.TPContext sums more than two bf16 partials in f32 and rounds once
(TPContext._sum_gloo), so a sum is within 2^-8 |sum| <= (W - 1) 2^-9 sum |a_i|.  With gloo's own bf16 adds -- W - 1 = 3
roundings of the running sum, half an ulp = 2^-8 of it each -- the same sums measured 1.27 - 1.68 of that bound (ar
1.512, mr 1.469, dh2 1.635, dh1 1.626, dhf sum 1.680).  RCCL's bf16 reduction over more than two GPUs is not run here.
"""
import json
import os
import types

import pytest
import torch

from tests import _dist

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GA = 4
B, S = 2, 128
CASES = {
    "sp_c2_L2": dict(tp=2, layers=2, over=dict(tp_sp=1, tp_sp_chunks=2)),
    "sp_c1": dict(tp=2, layers=1, over=dict(tp_sp=1, tp_sp_chunks=1)),
    "replicated": dict(tp=2, layers=1, over=dict(tp_sp=0, vp_ce=0)),
    "tp4": dict(tp=4, layers=1, nkv=4, over=dict(tp_sp=1, tp_sp_chunks=2)),
    "main_grad": dict(tp=2, layers=1, over=dict(tp_sp=1, tp_sp_chunks=2), main_grad=True),
    "owner": dict(tp=2, layers=1, over=dict(tp_sp=1, tp_sp_chunks=2), owner=True),
}
WORST = {}   # (case, role) -> worst ratio over the ranks, filled by the cases for the table


def _cfg(layers, nkv=2):
    return types.SimpleNamespace(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=nkv,
                                 vocab_size=512, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S)


def _build(cfg, tp):
    os.environ.update(FLASH_ATTEN="1", CONTEXT_PARALLEL="0")
    torch.cuda.set_device(0)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    from picotron_amd.tensor_parallel.tensor_parallel import apply_tensor_parallel
    m = pgm.setup_process_group_manager(tp_size=tp, cp_size=1, pp_size=1, dp_size=1)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = apply_tensor_parallel(Llama(cfg))
    model.to(BF)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:   # norm weights away from 1 (a dropped weight must show), the same on every rank
                p.copy_((1 + 0.1 * torch.randn(p.shape, generator=g)).to(p))
    return m, model


def _batch(cfg, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (B, S + 1), generator=g)
    tgt = ids[:, 1:].reshape(-1).clone()
    tgt[torch.randperm(tgt.numel(), generator=g)[:max(1, tgt.numel() // 20)]] = -100   # ~5 % ignored
    return ids[:, :-1].contiguous(), tgt


def _assert_form(name, spec, rec, model, cfg, T):
    """The form the case names was taken, from the recorder."""
    tp, L, H = spec["tp"], cfg.num_hidden_layers, cfg.hidden_size
    names = rec.names()
    colls = [k for k in rec.calls if T.is_coll(k)]
    count = lambda n: sum(k.name == n for k in colls)   # noqa: E731
    sp = spec["over"]["tp_sp"] != 0
    assert all(layer.tp_sequence_parallel == sp for layer in model.decoder_layers)
    if not sp:
        assert "residual_add" not in names and count("all_gather_rows_into") == 0 and count("reduce_scatter_rows_into") == 0
        assert "cross_entropy_vp_partial" not in names and "cross_entropy_loss_lse" in names
        assert count("all_reduce") == 4 * L + 1, count("all_reduce")   # a, m, dh2, dh1 per layer, the lm_head dX
        assert sum(not k.sync for k in colls) == 2 * L + 1             # the dX sums run beside the dW GEMMs
        return
    c = spec["over"]["tp_sp_chunks"]
    n = B * S // (c * tp)
    assert names.count("residual_add") == L and "cross_entropy_vp_partial" in names and "cross_entropy_loss_lse" not in names
    gathers = [k for k in colls if k.name == "all_gather_rows_into"]
    rows = [k for k in gathers if tuple(k.ins[0].key[1]) == (n, H)]
    assert len(rows) == c * (4 * L + 2) and len(gathers) == len(rows) + 1, (len(rows), len(gathers))   # + the CE's 16 B per row
    assert all(not k.sync for k in rows) and count("reduce_scatter_rows_into") == c * (4 * L + 1)
    ars = [k for k in colls if k.name == "all_reduce"]
    blocks = [tuple(k.ins[0].key[1]) for k in ars if k.ins[0].key[3] == F32]
    assert blocks == ([(1, H)] * (2 * L) if spec.get("owner") else [(2 * L, H)]), blocks   # immediate / one deferred block
    assert len(ars) == len(blocks) + 1   # + the lm_head dX
    assert ("rmsnorm_colsum_batch" in names)


def _case(rank, world, name, outdir):
    from picotron_amd import functional as FN
    from picotron_amd import kernels as K
    from picotron_amd import switches
    from tests import _model_ref as M
    from tests import _tp_ref as T
    spec = CASES[name]
    cfg = _cfg(spec["layers"], spec.get("nkv", 2))
    with switches.override(**spec["over"]):
        m, model = _build(cfg, spec["tp"])
        g = torch.Generator().manual_seed(9)
        for n, p in model.named_parameters():
            if spec.get("main_grad"):   # prior contents, the same on every rank for the replicated weights
                p.main_grad = (0.05 * torch.randn(p.shape, generator=g)).to(F32).cuda()
            if spec.get("owner") and "norm" in n:
                p._pt_grad_ready = lambda p: None
        ids, tgt = _batch(cfg)
        names = {id(p): n for n, p in model.named_parameters()}
        with M.recording() as rec, T.recording_collectives(rec, model, names):
            logits = model(ids.cuda())
            loss = FN.cross_entropy(logits.view(-1, cfg.vocab_size), tgt.cuda()) / GA
            loss.backward()
            torch.cuda.synchronize()
        _assert_form(name, spec, rec, model, cfg, T)
        sp = spec["over"]["tp_sp"] != 0
        c = spec["over"].get("tp_sp_chunks", 1)
        roles, cfgs, hc, ce_name, (wev, nev) = T.extract_tp(K, rec.calls, model, B, S, torch.ones((), dtype=BF) / GA,
                                                            spec["tp"], m.tp_rank, c, sp)
        assert ce_name == ("cross_entropy_vp_combine" if sp else "cross_entropy_loss_lse")
        allr = T.exchange(roles)
        over = None
        try:
            T.check_tp(allr, m.tp_rank, cfgs, hc, name)
        except AssertionError as e:   # sums over their bound: every other stage was checked; raised below, after the table's figures
            if not str(e).startswith("stage sums:"):
                raise
            over = e
        # the sinks of a chunked layer: chunk 0's launch and every later chunk's are separate events
        launches = T.check_notifications(rec.calls, wev, nev, sp)
        nc = c if sp else 1
        for n, evs in wev.items():
            want = nc if "decoder_layers" in n else 1
            assert len(evs) == want and launches[n] == want, f"{n}: {len(evs)} launches for {want} chunks"
            epis = [e["epi"] for e in evs]
            first = K.EPI_F32_ACC if spec.get("main_grad") else K.EPI_BF16
            rest = K.EPI_F32_ACC if spec.get("main_grad") else K.EPI_BF16_ACC
            assert epis == [first] + [rest] * (want - 1), f"{n}: epilogues {epis}"
        assert T.check_waits(rec.calls) > 0
        if spec.get("owner"):   # W = 2: the immediate and the deferred sum over tp give the same bits
            norms = {n: p for n, p in model.named_parameters() if "layernorm" in n}
            first = {n: p.grad.clone() for n, p in norms.items()}
            for p in model.parameters():
                p.grad = None
                if hasattr(p, "_pt_grad_ready"):
                    del p._pt_grad_ready
            with M.recording(clone=False) as plain:
                (FN.cross_entropy(model(ids.cuda()).view(-1, cfg.vocab_size), tgt.cuda()) / GA).backward()
                torch.cuda.synchronize()
            assert plain.names().count("rmsnorm_colsum_batch") == 2   # the deferred path: into the block, then into the sinks
            assert len(norms) == 2 * cfg.num_hidden_layers
            for n, p in norms.items():
                M._bits_equal(f"{n}: the deferred sum over tp against the immediate one", p.grad, first[n])
    worst = {f"{form}|{role}": v for (form, role), v in M.WORST.items() if form == name}
    with open(os.path.join(outdir, f"{name}_{rank}.json"), "w") as f:
        json.dump(worst, f)
    if over is not None:
        raise over
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_tp_form_every_stage_on_every_rank(name, tmp_path):
    tp = CASES[name]["tp"]
    try:
        _dist.run(_case, tp, name, str(tmp_path), device="cuda")
    finally:
        for rank in range(tp):
            if (tmp_path / f"{name}_{rank}.json").exists():
                with open(tmp_path / f"{name}_{rank}.json") as f:
                    for k, v in json.load(f).items():
                        role = k.split("|", 1)[1]
                        WORST[(name, role)] = max(WORST.get((name, role), 0.0), v)


def test_zz_worst_ratio_table():
    """Worst |got - ref| / bound per role (rows) and case (columns), over the ranks; '-': the case has no such role."""
    assert WORST, "no case ran before the table"
    cases = [c for c in CASES if any(k[0] == c for k in WORST)]
    roles = sorted({r for _, r in WORST})
    lines = ["    " + f"{'role':<34}" + "".join(f"{c:>11}" for c in cases)]
    for r in roles:
        lines.append("    " + f"{r:<34}" + "".join(f"{WORST[(c, r)]:>11.3f}" if (c, r) in WORST else f"{'-':>11}" for c in cases))
    print("\n" + "\n".join(lines))
    assert max(WORST.values()) <= 1.0
