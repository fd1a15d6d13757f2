"""A mixture-of-experts Llama on the GPU: train_step with the aux loss, the gradient sinks, weight-
gradient pairing, bit-identical repeats, MoE together with document ids and QK-norm against the
composed reference (tests/_model_ref.py's stage kit extended in tests/_moe_stage_ref.py; an fp32 oracle
composition beside it as a smoke check), and the dense path untouched."""
import types

import pytest
import torch

from oracle import picotron_oracle as O
from tests import _gemm_ref as G
from tests import _moe_model_ref as MR

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TOL = 2e-2
S, H, V, E = 64, 128, 256, 8
CFG = dict(hidden_size=H, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=V,
           rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=S, num_experts=E,
           num_experts_per_tok=2)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _model(seed=0, **over):
    from picotron_amd.model import Llama
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**dict(CFG, **over)))
    return model.to(BF)


def _is_moe_weight(name):
    return ".mlp.experts." in name or ".mlp.router." in name


def _train(steps, seed=0, main_grad=False, pair=1, coef=0.01):
    """`steps` train_steps (mbs 2, grad_acc 2) with AdamW; (model, losses, aux parts, last step's gradients)."""
    from picotron_amd import optim, switches
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    dev = torch.device("cuda")
    model = _model(seed)
    if main_grad:
        for p in model.parameters():
            p.main_grad = torch.zeros(p.shape, dtype=F32, device=dev)
    opt = None if main_grad else optim.AdamW(model.parameters(), lr=3e-3, weight_decay=0.0)
    loader = SyntheticMicroBatchDataLoader(2, S, 2, V, dev, seed=99)
    losses, auxes, grads = [], [], None
    with switches.override(wgrad_pair=pair):
        for _ in range(steps):
            losses.append(train_step(model, loader, dev, moe_aux_loss=coef))
            auxes.append(model.moe_aux_part.item())
            grads = {n: (p.main_grad if main_grad else p.grad).detach().clone() for n, p in model.named_parameters()}
            if opt is not None:
                opt.step()
                opt.zero_grad(set_to_none=True)
    return model, losses, auxes, grads


def test_train_step_with_aux_loss_trains_and_repeats():
    model, losses, auxes, grads = _train(8)
    print("moe train_step losses", [round(l, 4) for l in losses], "aux", [round(a, 4) for a in auxes])
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]
    # the Switch loss is >= 1 per layer (Cauchy-Schwarz on f and P, equality at uniform routing), less
    # rounding; the model sums its two MoE layers
    assert all(a == a and a >= 2 * (1 - 1e-3) for a in auxes)
    assert model.moe_aux_part.dtype == F32 and model.moe_aux_part.is_cuda and model.moe_aux_part.dim() == 0
    assert model.z_loss_part is None
    for n, g in grads.items():   # bf16 .grad: the sink wgrad_group picks without a DP owner
        if _is_moe_weight(n):
            assert g.dtype == BF and bool(torch.isfinite(g.float()).all()) and float(g.float().abs().sum()) > 0, n
    # two runs from the same seed: the same bits
    model2, losses2, auxes2, grads2 = _train(8)
    assert losses2 == losses and auxes2 == auxes
    for (n, p), q in zip(model.named_parameters(), model2.parameters()):
        assert torch.equal(p, q), n
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n


def test_main_grad_sinks_and_default_changes_nothing():
    """With an f32 main_grad on every parameter (what DataParallelBucket attaches) the expert and
    router gradients land there, p.grad stays unset; moe_aux_loss = 0 leaves no aux part and gives the
    plain cross-entropy loss."""
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    model, losses, auxes, grads = _train(1, main_grad=True)
    for n, p in model.named_parameters():
        if _is_moe_weight(n):
            assert p.grad is None and grads[n].dtype == F32 and float(grads[n].abs().sum()) > 0, n
    dev = torch.device("cuda")
    m = _model(0)
    loader = SyntheticMicroBatchDataLoader(2, S, 2, V, dev, seed=99)
    plain = train_step(m, loader, dev)
    assert m.moe_aux_part is None and m.moe_aux_loss is not None and m.moe_aux_loss.requires_grad
    router = "decoder_layers.0.mlp.router.weight"
    g_plain = dict(m.named_parameters())[router].grad.clone()
    m.zero_grad(set_to_none=True)
    with_aux = train_step(m, SyntheticMicroBatchDataLoader(2, S, 2, V, dev, seed=99), dev, moe_aux_loss=0.5)
    assert abs(with_aux - (plain + 0.5 * m.moe_aux_part.item())) < 5e-3 * abs(with_aux)   # (a bf16 loss: 2^-9)
    assert not torch.equal(dict(m.named_parameters())[router].grad, g_plain)   # the aux loss reaches the router
    with pytest.raises(ValueError, match="mixture-of-experts"):
        train_step(_model(0, num_experts=0), SyntheticMicroBatchDataLoader(2, S, 2, V, dev, seed=99), dev, moe_aux_loss=0.1)


BIG = dict(hidden_size=256, intermediate_size=256, num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=128)


def _pair_run(pair, seq=S, **over):
    """One train_step (mbs 2, grad_acc 2) on fresh weights with every MoE layer's stages of BOTH
    micro-batches and the sinks as they stood between them."""
    from picotron_amd import switches
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    dev = torch.device("cuda")
    model = _model(0, **over)
    moes = [l.mlp for l in model.decoder_layers]
    for m in moes:
        m.stages = {}
    snap = {}

    def between(i):
        if i == 1:
            snap["stages"] = [{k: v.cpu() for k, v in m.stages.items()} for m in moes]
            snap["grads"] = {n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in model.named_parameters()}
    with switches.override(wgrad_pair=pair):
        loss = train_step(model, SyntheticMicroBatchDataLoader(2, seq, 2, V, dev, seed=99), dev, on_microbatch=between,
                          moe_aux_loss=0.01)
    second = [{k: v.cpu() for k, v in m.stages.items()} for m in moes]
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    return loss, snap, second, grads


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


def test_weight_gradient_pairing_on_and_off_bit_equal():
    """grad_acc = 2 with weight-gradient pairing on and off: bit-equal losses, stages and gradients.
    At hidden 128 no weight gradient of the model tiles by the 256 x 256 kernel the K = 2 T launch
    needs, so a completed pair runs as its two halves -- a store, then an accumulating launch, the
    summation order of the unpaired path (the next test covers shapes that do pair)."""
    loss_p, snap_p, st2_p, g_p = _pair_run(1)
    loss_u, snap_u, st2_u, g_u = _pair_run(0)
    assert loss_p == loss_u
    for layer in range(2):
        for a, b in ((snap_p["stages"][layer], snap_u["stages"][layer]), (st2_p[layer], st2_u[layer])):
            assert set(a) == set(b)
            for n in a:
                assert _same_bits(a[n], b[n]), n
    for n in g_p:
        assert torch.equal(g_p[n], g_u[n]), n
    moe = [n for n in g_p if _is_moe_weight(n)]
    assert len(moe) == 2 * (3 * E + 1)
    assert all(snap_p["grads"][n] is None for n in moe)       # pairing on: the first micro-batch deferred them
    assert all(snap_u["grads"][n] is not None for n in moe)   # pairing off: it wrote them


def test_weight_gradient_pairing_where_it_changes_the_summation():
    """hidden = intermediate = 256, 256 tokens per micro-batch (C = 128): the experts' weight
    gradients tile by 256 x 256 and a pair is ONE K = 2 C launch.  That changes the summation --
    bf16(a + b) from one f32 accumulator against bf16(bf16(a) + bf16(b)) -- so the results are not
    bit-equal, and each is held to tests/_gemm_ref.py's per-element rule on its own operands: the
    paired sink as the bf16 store of the K-concatenated product, the unpaired one as EPI_BF16_ACC of
    the second micro-batch's product onto the sink as it stood after the first.  The router's
    gradient ([8, 256]: off the 64-grid) runs as two halves either way and stays bit-equal, like the
    loss and every forward stage."""
    from picotron_amd import kernels as K
    loss_p, snap_p, st2_p, g_p = _pair_run(1, seq=128, **BIG)
    loss_u, snap_u, st2_u, g_u = _pair_run(0, seq=128, **BIG)
    assert loss_p == loss_u
    C = K.moe_capacity(256, E, 2, 1.25)
    I = BIG["intermediate_size"]
    assert C == 128
    differs = 0
    for layer in range(2):
        a_p, b_p, a_u, b_u = snap_p["stages"][layer], st2_p[layer], snap_u["stages"][layer], st2_u[layer]
        for n in ("logits", "idx", "slot", "out"):
            assert _same_bits(a_p[n], a_u[n]) and _same_bits(b_p[n], b_u[n]), n
        pre = f"decoder_layers.{layer}.mlp."
        assert torch.equal(g_p[pre + "router.weight"], g_u[pre + "router.weight"])
        jobs = []
        for e in range(E):
            rows = slice(e * C, (e + 1) * C)
            jobs += [(f"{pre}experts.{e}.down_proj.weight", lambda s, r=rows: s["dye"][r], lambda s, r=rows: s["hh"][r]),
                     (f"{pre}experts.{e}.gate_proj.weight", lambda s, r=rows: s["dgu"][r, :I], lambda s, r=rows: s["xe"][r]),
                     (f"{pre}experts.{e}.up_proj.weight", lambda s, r=rows: s["dgu"][r, I:], lambda s, r=rows: s["xe"][r])]
        for name, dy, x in jobs:
            assert snap_p["grads"][name] is None        # paired: nothing was written after the first micro-batch
            acc, Sabs = G.ref_product(torch.cat([dy(a_p), dy(b_p)]).t(), torch.cat([x(a_p), x(b_p)]))
            t, bound = G.target_and_bound(acc, Sabs, 2 * C, G.EPI_BF16)
            G.check(f"paired {name}", g_p[name], t, bound, tag="moe-pair")
            acc, Sabs = G.ref_product(dy(b_u).t(), x(b_u))
            t, bound = G.target_and_bound(acc, Sabs, C, G.EPI_BF16_ACC, old=snap_u["grads"][name])
            G.check(f"unpaired {name}", g_u[name], t, bound, tag="moe-pair")
            differs += int(not torch.equal(g_p[name], g_u[name]))
    print(f"pairing: {differs} of {2 * 3 * E} expert gradients differ by bits between the two forms")
    assert differs > 0   # the K = 2 C launch did run


def _doc_layer():
    """A MoE decoder layer with QK-norm (norm weights off 1) and a batch of packed rows: documents of uneven
    length, a boundary inside a 64-key tile and one at a tile edge.  (layer, x, dy, document ids, mask, B, S)."""
    from picotron_amd.model import DecoderLayer, MoE
    B, Sq = 2, 128
    torch.manual_seed(3)
    with torch.device("cuda"):
        layer = DecoderLayer(types.SimpleNamespace(**dict(CFG, qk_norm=True, max_position_embeddings=Sq)), 0)
    layer.to(BF)
    assert isinstance(layer.mlp, MoE)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if p.dim() == 1:
                p.copy_((1 + 0.25 * torch.randn(p.shape, generator=g)).to(p.dtype))
    docs = torch.zeros(B, Sq, dtype=torch.long)
    docs[0, 37:] = 1
    docs[0, 64:] = 2
    docs[1, 100:] = 1
    i = torch.arange(Sq)
    mask = (i[None, :] <= i[:, None])[None, None] & (docs[:, :, None] == docs[:, None, :])[:, None]
    x, dy = torch.randn(B, Sq, H, generator=g).to(BF), torch.randn(B, Sq, H, generator=g).to(BF)
    return layer, x, dy, docs, mask, B, Sq


def test_moe_layer_with_document_ids_and_qk_norm_every_stage():
    """Document ids and QK-norm together with MoE against the composed reference: tests/_model_ref.py's
    recorded, teacher-forced stage kit, extended in tests/_moe_stage_ref.py.  The layer's kernel calls are
    recorded; the kit's own extraction reads the attention block (band, QK-norm, their bit-identity replays)
    and the norms from the trace, the MoE's stages complete the roles, and EVERY role of the forward and the
    backward -- weight gradients included -- is held per element to its kernel kit's bound."""
    from picotron_amd import kernels as K
    from tests import _model_ref as M
    from tests import _moe_stage_ref as MS
    layer, x, dy, docs, mask, B, Sq = _doc_layer()
    layer.mlp.stages = {}
    d_aux = 0.5
    xg = x.cuda().requires_grad_(True)
    with M.recording() as rec:
        y = layer(xg, document_ids=docs.cuda())
        torch.autograd.backward([y, layer.mlp.aux_loss], [dy.cuda(), torch.tensor(d_aux, device="cuda")])
        torch.cuda.synchronize()
    names = rec.names()
    assert all(c.kwargs.get("band") is not None for c in rec.calls if c.name in ("attn_fwd", "attn_bwd"))
    assert "qk_norm_rope_fwd" in names and "qk_norm_bwd" in names and "linear_fwd_rope" not in names
    for n in ("moe_route", "moe_plan", "moe_dispatch", "moe_experts_fwd", "moe_combine", "moe_combine_bwd", "moe_route_bwd"):
        assert n in names, n
    c = MS.moe_layer_config(layer, B, Sq, mask=mask, d_aux=d_aux)
    r = MS.extract_moe_layer(K, layer, rec.calls, c, y, xg.grad)
    stages = MS.moe_layer_stages(c)
    res = M.check_stages(r, c, stages, "moe docmask qk_norm")
    assert set(res) == {"/".join(s.produces) or "dW_qkv" for s in stages}   # every stage was checked
    for must in ("qk_normed/rstd_qk", "o/lse", "dqkv", "dqkv_unrot", "m_idx/m_gate/m_probs/m_counts/m_aux", "out", "dh2",
                 "m_dW_d/m_dW_g/m_dW_u", "dz", "dx1", "dx"):
        assert must in res, must
    print(M.worst_table(full=False))


def test_moe_layer_with_document_ids_and_qk_norm_beside_the_fp32_oracle():
    """A smoke check beside the per-stage test above: the whole layer against an fp32 composition of the oracle's
    ops (tests/_moe_model_ref.py) by norm-relative error -- it ties the stage kit's teacher-forced roles to an
    independent end-to-end evaluation, and shows the mask arrived."""
    layer, x, dy, docs, mask, B, Sq = _doc_layer()
    nh, nkv, d = 2, 2, 64
    layer.mlp.stages = {}
    xg = x.cuda().requires_grad_(True)
    y = layer(xg, document_ids=docs.cuda())
    aux = layer.mlp.aux_loss
    torch.autograd.backward([y, aux], [dy.cuda(), torch.tensor(0.5, device="cuda")])
    st = {k: v.cpu() for k, v in layer.mlp.stages.items()}
    p = {k: v.detach().float().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    xr = x.float().requires_grad_(True)
    cos, sin = (t.float() for t in O.get_cos_sin(Sq, d, base=10000.0))
    yr, auxr = MR.ref_moe_decoder_layer(xr, p, cos, sin, nh, nkv, 1e-5, O.rmsnorm_flash_semantics, st["idx"].long(),
                                        st["slot"] >= 0, mask=mask)
    torch.autograd.backward([yr, auxr], [dy.float(), torch.tensor(0.5)])
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), "aux": abs(aux.item() - auxr.item()) / auxr.item(),
            **{n: rel(t.grad, p[n].grad) for n, t in layer.named_parameters()}}
    print("moe + document ids + qk-norm: worst", max(errs.values()), max(errs, key=errs.get))
    assert max(errs.values()) < TOL, errs
    # the mask arrived: without it the output is well outside the tolerance
    y_plain = layer(x.cuda())
    assert rel(y_plain, yr) > 2 * TOL


DP_SEED, DP_COEF = 99, 0.01


def _dp2(rank, world, want):
    """train_step under DataParallelBucket (f32 main_grad, the bucket all-reduce on the last micro-batch), each
    rank its own tokens; the aux loss reaches the module through the wrapper."""
    import os
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.data_parallel.data_parallel import DataParallelBucket
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=world)
    dev = torch.device("cuda")
    model = _model(0)
    ddp = DataParallelBucket(model)
    loss = train_step(ddp, SyntheticMicroBatchDataLoader(2, S, 2, V, dev, seed=DP_SEED), dev, moe_aux_loss=DP_COEF)
    torch.cuda.synchronize()
    assert loss == loss and ddp.moe_aux_part.item() >= 2 * (1 - 1e-3)
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == BF, n
        assert rel(p.grad, want[n]) < TOL, n


def test_data_parallel_bucket_dp2_with_aux_loss():
    """dp = 2: every gradient, the experts' and the router's included, is the one-process run's over both
    ranks' micro-batches (their mean), aux loss and all."""
    from tests import _dist
    from picotron_amd import functional as FN
    dp, ga = 2, 2
    model = _model(0)
    tokens = torch.randint(0, V, (dp, ga, 2, S + 1), generator=torch.Generator().manual_seed(DP_SEED))   # the loader's draw
    for p in model.parameters():
        p.main_grad = torch.zeros(p.shape, dtype=F32, device="cuda")
    for r in range(dp):
        for i in range(ga):
            t = tokens[r, i]
            lo = model(t[:, :-1].cuda())
            ce = FN.cross_entropy(lo.view(-1, V), t[:, 1:].reshape(-1).cuda())
            ((ce + DP_COEF * model.moe_aux_loss) / (ga * dp)).backward()
    want = {n: p.main_grad.detach().cpu() for n, p in model.named_parameters()}
    torch.cuda.synchronize()
    _dist.run(_dp2, dp, want, device="cuda")


def test_dense_config_takes_the_dense_node_bit_for_bit():
    """A config without experts builds today's layer: DecoderLayerFunction is the node, the output equals
    a direct call of it with the layer's own arguments by bits, and the model leaves no aux loss."""
    from picotron_amd import functional as FN
    from picotron_amd.model import MLP, _norm_eps, _norm_mode
    model = _model(0, num_experts=0)
    assert all(type(l.mlp) is MLP for l in model.decoder_layers)
    ids = torch.randint(0, V, (2, S), generator=torch.Generator().manual_seed(1)).cuda()
    logits = model(ids)
    assert model.moe_aux_loss is None
    layer = model.decoder_layers[0]
    x = torch.randn(2, S, H, generator=torch.Generator().manual_seed(2)).to(BF).cuda().requires_grad_(True)
    y = layer(x)
    assert type(y.grad_fn).__name__ == "DecoderLayerFunctionBackward"
    n1, n2, at, mlp = layer.input_layernorm, layer.post_attention_layernorm, layer.attention, layer.mlp
    cos, sin = layer._tables(x.device)
    want = FN.DecoderLayerFunction.apply(x, n1.weight, n2.weight, *at.weights(), mlp.gate_proj.weight, mlp.up_proj.weight,
                                         mlp.down_proj.weight, cos, sin, _norm_eps(n1), _norm_mode(n1), at.num_local_heads,
                                         at.num_local_kv_heads, at.head_dim, False, 0, None)
    assert torch.equal(y, want)
    moe_y = _model(0).decoder_layers[0](x)
    assert type(moe_y.grad_fn).__name__ == "MoEFunctionBackward"
    assert logits.shape == (2, S, V)
