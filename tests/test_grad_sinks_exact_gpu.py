"""Bit-for-bit identities of the gradient sinks (picotron_amd/functional.py: _wgrad_target, _norm_dw_sink, the
deferred norm column sums, the embedding sink, the paired weight gradients) on the tiny 2-layer Llama (B 2, S 128,
H 256, I 512, heads 4 / 2 of 64, V 512, with QK-norm): a token-embedding gradient, every norm weight, the seven
projections of each layer and the head.  Variant `shared`: one Parameter is the input_layernorm weight of both
layers.

Notation: g_i = micro-batch i alone from .grad = None; f_i = the same into a zeroed f32 main_grad; b_i = the same
into a zeroed bf16 main_grad.  The header fixes the sinks (EPI_BF16_ACC = bf16(old + bf16(acc)), EPI_F32_ACC =
old + acc, PT_DW_ACC_* likewise) and wgrad_form is a pure function of the shapes, the sinks' alignment and the
switches, so for every parameter, by bits:

  1. bf16(f_i) == g_i == b_i
  2. two and three micro-batches accumulated into bf16 .grad == bf16(bf16(g_1 + g_2) + g_3), computed on the
     host from the stored bits; the same from a pre-filled .grad
  3. f32 main_grad after three micro-batches == (f_1 + f_2) + f_3 in f32
  4. mixed sinks (.grad pre-filled / None / frozen, one or two of q | k | v frozen): every trainable parameter as
     in 1 and 2, a frozen .grad stays None, a pre-filled frozen .grad keeps its bits
  5. norm_defer = 0 and 1: identical bits for every gradient
  6. train_step with ga = 2, 3, 4 and wgrad_pair = 1: no pending pair, phase None, no pending norm sums, no CE
     statistics stashed afterwards; every paired launch passes the GEMM stage check with both micro-batches'
     recorded operands (K = 2 T) onto the sink's prior contents, and those operands are, by bits, the roles of
     the deferring micro-batch; the unpaired odd micro-batch passes the plain check; wgrad_pair = 0 on the same
     data satisfies identity 2.

Replaced by the stage check (tests/_model_ref.py), with the reason:
  * the shared input_layernorm weight in identities 2 and 3: its gradient is two contributions per micro-batch,
    stored / accumulated one after the other (functional._flush_norm_dw's generations), so the sink after two
    micro-batches is bf16(bf16(G + c_a) + c_b), which is not a function of G and g_2 = bf16(c_a + c_b) alone.
    For the same reason bf16(f_i) == g_i is not claimed for it (f32: the two contributions' sum rounded once;
    bf16: each rounded, then their sum); b_i == g_i and identity 5 hold for it by bits; in 2 and 3 each of its
    contributions is held to the norm kit's dweight bound onto the recorded prior contents.
  * the q | k | v + out_proj group under pairing (identity 6): k_proj and v_proj have 128 rows, the K-segmented
    256 x 256 tile takes only sinks whose row boundaries are multiples of 256 (picotron_amd/csrc/gemm.hip args_fit), and
    kernels._wgrad_grouped_launch then runs the whole group as kernels._wgrad_unpaired documents: the first
    micro-batch's half through the sink's epilogue, the second's accumulating onto it.  That is two roundings
    where the K = 2 T launch has one, so these four sinks are held to the two launches' GEMM bounds in sequence
    (_model_ref._wgrad_unpaired) instead of the single K = 2 T bound; down_proj, gate|up and the head (256- and
    512-row sinks) run paired and are held to the K = 2 T bound.
"""
import types

import pytest
import torch

from tests import _model_ref as M

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GA, NMB = 3, 3


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    yield
    from picotron_amd import functional as FN
    FN._CE_STATS.clear()


def K_():
    from picotron_amd import kernels
    return kernels


def cfg_tiny(layers=2, V=512, S=128):
    return types.SimpleNamespace(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                                 vocab_size=V, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S, qk_norm=True)


def build(shared):
    from picotron_amd.model import Llama
    cfg = cfg_tiny()
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:
                p.copy_(1 + 0.1 * torch.randn_like(p))
    if shared:
        model.decoder_layers[1].input_layernorm.weight = model.decoder_layers[0].input_layernorm.weight
    return model, cfg


def batches(cfg, n=NMB, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ids = torch.randint(0, cfg.vocab_size, (2, cfg.max_position_embeddings + 1), generator=g)
        tgt = ids[:, 1:].reshape(-1).clone()
        tgt[::23] = -100
        out.append((ids[:, :-1].contiguous().cuda(), tgt.cuda()))
    return out


def micro(model, cfg, mb, ga=GA):
    from picotron_amd import functional as FN
    ids, tgt = mb
    (FN.cross_entropy(model(ids).view(-1, cfg.vocab_size), tgt) / ga).backward()


def reset(model, main=None, fill=None):
    """Every sink back to its start: .grad None (or pre-filled with fill[name]), main_grad removed or zeroed in `main`."""
    for n, p in model.named_parameters():
        p.grad = None if fill is None or n not in fill else fill[n].clone().cuda()
        if main is None:
            if hasattr(p, "main_grad"):
                del p.main_grad
        else:
            p.main_grad = torch.zeros_like(p, dtype=main)


def sinks(model):
    torch.cuda.synchronize()
    out = {}
    for n, p in model.named_parameters():
        g = getattr(p, "main_grad", None)
        g = p.grad if g is None else g
        out[n] = None if g is None else g.detach().cpu().clone()
    return out


def same(name, got, want, what):
    assert got is not None, f"{what}: {name} has no gradient"
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {name} {got.dtype} {tuple(got.shape)}"
    diff = M.R.ibits(got) != M.R.ibits(want)
    if bool(diff.any()):
        i = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {name}: {int(diff.sum())} of {diff.numel()} elements differ by bits; first at {i}: "
                             f"got {float(got[i])!r} want {float(want[i])!r}")


def acc_bf16(*gs):
    """bf16(bf16(g_0 + g_1) + g_2) ...: the bf16 sinks' accumulation, on the host from the stored bits."""
    it = list(gs)
    tot = it.pop(0)
    for g in it:
        tot = (tot.to(F32) + g.to(F32)).to(BF)
    return tot


@pytest.fixture(scope="module", params=["plain", "shared"])
def world(request):
    """(model, cfg, micro-batches, g, f, b, the shared weight's name or None): the three single-micro-batch
    references of every parameter, computed once.  A module-scoped fixture runs before the function-scoped
    autouse `_env` (and cannot use its monkeypatch), so it sets the same environment by hand for the model's
    construction and puts back what it found; every test then runs under `_env`'s own settings."""
    import os
    keep = {k: os.environ.get(k) for k in ("DEVICE", "LOCAL_RANK", "CONTEXT_PARALLEL", "FLASH_ATTEN")}
    os.environ.update(DEVICE="cuda", LOCAL_RANK="0", CONTEXT_PARALLEL="0", FLASH_ATTEN="1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    shared = request.param == "shared"
    model, cfg = build(shared)
    mbs = batches(cfg)
    g, f, b = [], [], []
    for mb in mbs:
        for store, main in ((g, None), (f, F32), (b, BF)):
            reset(model, main)
            micro(model, cfg, mb)
            store.append(sinks(model))
    reset(model)
    for k, v in keep.items():   # (each test sets its own through the autouse fixture)
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return model, cfg, mbs, g, f, b, ("decoder_layers.0.input_layernorm.weight" if shared else None)


def _stage_check_shared(rec, model, cfg, shared, form, n):
    """The replaced identity: every contribution to the shared norm weight under the norm kit's bound."""
    starts = [i for i, c in enumerate(rec.calls) if c.name == "embedding_fwd"]
    assert len(starts) == n
    for k, at in enumerate(starts):
        layers, hc, h, _ = M.extract_model(K_(), rec.calls, model, 2, cfg.max_position_embeddings,
                                           torch.ones((), dtype=BF) / GA, at=at)
        for c, r in layers:
            M.check_stages(r, c, M.layer_stages(c), f"{form} mb{k}", only=("dx",))


def test_1_store_equals_accumulate_onto_zero(world):
    model, cfg, mbs, g, f, b, shared = world
    assert len(g[0]) == (2 * 11 + 3 - (1 if shared else 0))   # embedding, 2 x (2 norms, 2 qk norms, 7 projections), final norm, head
    for i in range(NMB):
        for n in g[i]:
            assert f[i][n].dtype == F32 and b[i][n].dtype == BF
            if n != shared:   # (f32: (c_b + c_a) rounded once; bf16: each contribution rounded, then their sum)
                same(n, f[i][n].to(BF), g[i][n], f"identity 1, micro-batch {i}: bf16(f) == g")
            same(n, b[i][n], g[i][n], f"identity 1, micro-batch {i}: b == g")


@pytest.mark.parametrize("prefilled", [False, True])
def test_2_bf16_accumulation(world, prefilled):
    model, cfg, mbs, g, f, b, shared = world
    gen = torch.Generator().manual_seed(5)
    fill = {n: (0.01 * torch.randn(t.shape, generator=gen)).to(BF) for n, t in g[0].items()} if prefilled else None
    reset(model, fill=fill)
    with M.recording() as rec:
        for k, mb in enumerate(mbs):
            micro(model, cfg, mb)
            got = sinks(model)
            for n in g[0]:
                if n == shared:
                    continue
                want = acc_bf16(*([fill[n]] if prefilled else []), *[g[i][n] for i in range(k + 1)])
                same(n, got[n], want, f"identity 2 after {k + 1} micro-batches (prefilled={prefilled})")
    if shared:
        _stage_check_shared(rec, model, cfg, shared, "sinks bf16", NMB)
    reset(model)


def test_3_f32_main_grad_accumulation(world):
    model, cfg, mbs, g, f, b, shared = world
    reset(model, F32)
    with M.recording() as rec:
        for mb in mbs:
            micro(model, cfg, mb)
    got = sinks(model)
    for n in g[0]:
        if n != shared:
            same(n, got[n], (f[0][n] + f[1][n]) + f[2][n], "identity 3: (f_1 + f_2) + f_3")
    assert all(p.grad is None for p in model.parameters())
    if shared:
        _stage_check_shared(rec, model, cfg, shared, "sinks f32", NMB)
    reset(model)


MIXED = {
    # name fragments -> state; everything else: .grad None, trainable
    "q_frozen": dict(frozen=("layers.0.attention.q_proj",), prefilled=("k_proj", "mlp.up_proj", "final_norm"), frozen_filled=()),
    "kv_frozen": dict(frozen=("attention.k_proj", "attention.v_proj", "layers.1.mlp.down_proj", "post_attention_layernorm"),
                      prefilled=("q_proj", "gate_proj", "embedding", "q_norm"), frozen_filled=("attention.v_proj",)),
    "norms_head": dict(frozen=("layers.0.mlp.gate_proj", "k_norm", "final_proj"), prefilled=("out_proj", "input_layernorm"),
                       frozen_filled=("final_proj",)),
}


@pytest.mark.parametrize("case", list(MIXED))
def test_4_mixed_sinks(world, case):
    model, cfg, mbs, g, f, b, shared = world
    spec = MIXED[case]
    hit = lambda n, frags: any(s in n for s in frags)   # noqa: E731
    gen = torch.Generator().manual_seed(6)
    fill = {}
    for n, p in model.named_parameters():
        if hit(n, spec["prefilled"]) and not hit(n, spec["frozen"]) or hit(n, spec["frozen_filled"]):
            fill[n] = (0.01 * torch.randn(p.shape, generator=gen)).to(BF)
    reset(model, fill=fill)
    try:
        for n, p in model.named_parameters():
            p.requires_grad_(not hit(n, spec["frozen"]))
        for k in range(2):   # the second micro-batch accumulates through the same per-parameter launch forms
            micro(model, cfg, mbs[k])
            got = sinks(model)
            for n in g[0]:
                if hit(n, spec["frozen"]):
                    if n in fill:
                        same(n, got[n], fill[n], f"identity 4 ({case}): a pre-filled frozen .grad keeps its bits")
                    else:
                        assert got[n] is None, f"identity 4 ({case}): the frozen {n} got a gradient"
                elif n == shared and (n in fill or k):
                    continue   # two contributions onto a prior value: see the module docstring
                else:
                    want = acc_bf16(*([fill[n]] if n in fill else []), *[g[i][n] for i in range(k + 1)])
                    same(n, got[n], want, f"identity 4 ({case}) after {k + 1} micro-batches")
    finally:
        for p in model.parameters():
            p.requires_grad_(True)
        reset(model)


def test_5_norm_defer_switch(world):
    from picotron_amd import switches
    model, cfg, mbs, g, f, b, shared = world
    res = {}
    for defer in (1, 0):
        reset(model)
        with switches.override(norm_defer=defer), M.recording(clone=False) as rec:
            micro(model, cfg, mbs[0])
            one = sinks(model)
            micro(model, cfg, mbs[1])
            two = sinks(model)
        # off: one sum per QK-norm weight, layer and micro-batch (they have no fused sink); on: one launch per
        # width (H, head_dim) and per generation of a shared sink, at the end of each backward
        assert rec.names().count("rmsnorm_colsum_batch") == (2 * (2 + bool(shared)) if defer else 2 * 2 * 2)
        res[defer] = (one, two)
    for n in g[0]:
        same(n, res[0][0][n], res[1][0][n], "identity 5: norm_defer 0 == 1, one micro-batch")
        same(n, res[0][0][n], g[0][n], "identity 5: == g_1")
        same(n, res[0][1][n], res[1][1][n], "identity 5: norm_defer 0 == 1, two micro-batches")
    reset(model)


# the operands (dY, X) of each weight-gradient role as roles of the micro-batch that computed them
def _pair_operands(c, r, h):
    T, I, wq, wkv = c.B * c.S, c.I, c.nh * c.d, c.nkv * c.d
    dqkv = r["dqkv"]
    return {"dW_d": (r["dout"], r["hh"]), "dW_g": (r["dgu"][:, :I], r["h2"]), "dW_u": (r["dgu"][:, I:], r["h2"]),
            "dW_o": (r["dz"], r["o"].reshape(T, -1)), "dW_q": (dqkv[:, :wq], r["h1"]),
            "dW_k": (dqkv[:, wq:wq + wkv], r["h1"]), "dW_v": (dqkv[:, wq + wkv:], r["h1"])}


@pytest.mark.parametrize("ga", [2, 3, 4])
def test_6_train_step_pairing(world, ga):
    from picotron_amd import functional as FN
    from picotron_amd import switches
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    model, cfg, _, _, _, _, shared = world
    dev = torch.device("cuda")
    S = cfg.max_position_embeddings
    gloss = torch.ones((), dtype=BF) / ga

    def loader():
        return SyntheticMicroBatchDataLoader(2, S, ga, cfg.vocab_size, dev, seed=77)

    # g_i of the loader's micro-batches (loss / ga), each alone
    ld = loader()
    alone = []
    for i in range(ga):
        reset(model)
        micro(model, cfg, (ld._inputs[i], ld._targets[i].reshape(-1)), ga)
        alone.append(sinks(model))
    # wgrad_pair = 0: identity 2
    reset(model)
    with switches.override(wgrad_pair=0):
        train_step(model, loader(), dev)
    got = sinks(model)
    for n in got:
        if n != shared:
            same(n, got[n], acc_bf16(*[a[n] for a in alone]), f"identity 6 (ga {ga}): wgrad_pair = 0 is identity 2")
    # wgrad_pair = 1
    reset(model)
    K = K_()
    fell_back, real_unpaired = set(), K._wgrad_unpaired   # the sinks of every group that ran as two launches

    def spy(jobs, epilogue):
        fell_back.update(o.data_ptr() for _, _, outs in jobs for o in outs)
        return real_unpaired(jobs, epilogue)
    K._wgrad_unpaired = spy
    try:
        with switches.override(wgrad_pair=1), M.recording() as rec:
            train_step(model, loader(), dev)
            torch.cuda.synchronize()
    finally:
        K._wgrad_unpaired = real_unpaired
    ptr_of = {n: p.grad.data_ptr() for n, p in model.named_parameters()}
    assert FN.WgradPairing.pending == {} and FN.WgradPairing.phase is None
    assert FN._PENDING_DW == {} and FN._CE_STATS == {}
    starts = [i for i, c in enumerate(rec.calls) if c.name == "embedding_fwd"]
    assert len(starts) == ga
    prev = None
    for i, at in enumerate(starts):
        deferring = i % 2 == 0 and i + 1 < ga
        layers, hc, h, _ = M.extract_model(K, rec.calls, model, 2, S, gloss, at=at, wgrads=not deferring)
        form = f"pair ga{ga} mb{i}"
        if deferring:
            prev = (layers, h)
            continue
        paired = i % 2 == 1
        for li, (c, r) in enumerate(layers):
            ops = _pair_operands(*prev[0][li], None) if paired else None
            for role in ("dW_d", "dW_g", "dW_u", "dW_o", "dW_q", "dW_k", "dW_v"):
                assert ("prev" in r[role]) == paired, f"{form}: {role} {'is not' if paired else 'is'} a K = 2 T launch"
                if paired:   # the other half's operands are the deferring micro-batch's roles, by bits
                    # which bound applies rests on what ran: the spy on kernels._wgrad_unpaired saw this sink, or not
                    pname = M.layer_names(model, li)["w" + role[-1]]
                    assert bool(r[role]["unpaired"]) == (ptr_of[pname] in fell_back), f"{form}: {role} ({pname})"
                    assert bool(r[role]["unpaired"]) == (role in ("dW_o", "dW_q", "dW_k", "dW_v")), f"{form}: {role}"
                    M._bits_equal(f"{form} L{li} {role}: the pair's first dY", r[role]["prev"][0], ops[role][0])
                    M._bits_equal(f"{form} L{li} {role}: the pair's first X", r[role]["prev"][1], ops[role][1])
            M.check_stages(r, c, M.layer_stages(c), form, only=("dW_d", "dW_g", "dW_o", "dW_qkv"))
        assert ("prev" in h["dW_lm"]) == paired and ptr_of["final_proj.weight"] not in fell_back
        if paired:
            M._bits_equal(f"{form} dW_lm: the pair's first dY", h["dW_lm"]["prev"][0], prev[1]["dlogits"])
            M._bits_equal(f"{form} dW_lm: the pair's first X", h["dW_lm"]["prev"][1], prev[1]["hf"])
        M.check_stages(h, hc, M.HEAD_BWD, form, only=("dW_lm",))
    reset(model)


def test_6_displaced_pair(world):
    """A micro-batch that deferred its weight gradients and whose keys are deferred again (phases 0, 0, 1) is not
    lost: pair_jobs launches it on its own -- the sinks then hold g_1 by bits -- and the next two micro-batches
    pair onto it (EPI_BF16_ACC onto exactly those bits, under the stage check)."""
    from picotron_amd import functional as FN
    model, cfg, mbs, g, f, b, shared = world
    K = K_()
    reset(model)
    gemm = [n for n, p in model.named_parameters() if p.dim() == 2 and "embedding" not in n]
    try:
        with M.recording() as rec:
            for mb, phase in zip(mbs, (0, 0, 1)):
                FN.wgrad_pairing(phase)
                micro(model, cfg, mb)
            torch.cuda.synchronize()
    finally:
        FN.wgrad_pairing(None)
        FN.flush_wgrad_pairs()
    assert FN.WgradPairing.pending == {} and FN._PENDING_DW == {}
    wev = M.sink_events(rec.calls, M.grad_sinks(model))
    for n in gemm:
        ev = wev[n]
        assert len(ev) == 2, f"{n}: {len(ev)} weight-gradient launches, the displaced one and the pair make 2"
        assert not isinstance(ev[0]["dy"], M.Pair) and ev[0]["epi"] == K.EPI_BF16
        same(n, ev[0]["got"], g[0][n], "the displaced micro-batch, launched on its own, is g_1")
        assert isinstance(ev[1]["dy"], M.Pair) and ev[1]["epi"] == K.EPI_BF16_ACC
        same(n, ev[1]["old"], g[0][n], "the pair accumulates onto g_1")
    starts = [i for i, c in enumerate(rec.calls) if c.name == "embedding_fwd"]
    layers, hc, h, _ = M.extract_model(K, rec.calls, model, 2, cfg.max_position_embeddings, torch.ones((), dtype=BF) / GA,
                                       at=starts[2])
    for c, r in layers:
        M.check_stages(r, c, M.layer_stages(c), "pair displaced", only=("dW_d", "dW_g", "dW_o", "dW_qkv"))
    M.check_stages(h, hc, M.HEAD_BWD, "pair displaced", only=("dW_lm",))
    reset(model)
