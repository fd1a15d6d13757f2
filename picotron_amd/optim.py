"""AdamW for the training step (reference train.py:205-209: `torch.optim.AdamW(model.parameters(),
lr=learning_rate)`), with each tensor's update fused into one HIP pass (csrc/adamw.hip).

Same constructor, defaults, param_groups and state layout as torch.optim.AdamW (state['step'] a CPU
float tensor, state['exp_avg'] / state['exp_avg_sq'] in the parameter's dtype), so a checkpoint of
one loads into the other; the per-element math is torch's multi-tensor (foreach) Adam with
decoupled weight decay, op for op with the same roundings to the storage dtype.

Global gradient-norm clipping (what a Llama recipe puts between the backward and the step,
torch.nn.utils.clip_grad_norm_) is part of the step: AdamW(..., max_grad_norm=M), or the stand-alone
clip_grad_norm_ below.  Both compute ONE norm for the whole model -- over tensor- and pipeline-
parallel ranks too -- in f32 on the device, and nothing of it is read on the host.

AdamW(..., master_weights=True) is the mixed-precision recipe on top (opt-in; not torch's layout): an
f32 `master_param` and f32 moments in the state of every bf16 parameter, one multi-tensor launch.

AdamW(..., stochastic_rounding=True) is the recipe in between (opt-in; torch's layout): bf16 state, the
update in f32 registers, and the three stores rounded up or down with probability equal to the
discarded fraction, on counter-based random bits that a resumed run reproduces.

Muon (torch.optim.Muon's interface; csrc/muon.hip + the GEMM launch layer) steps the decoder layers'
2-D matrices; MuonAdamW pairs it with AdamW for everything else under one global gradient norm, and
split_muon_params says which parameter goes where.
"""
import itertools

import torch
import torch.distributed as dist

from . import kernels as K
from . import process_group_manager as pgm


def grad_norm_plan(params, tp_size, pp_size):
    """How the global gradient norm is put together on a (tp, pp) grid; pure.  Returns
    (sharded, replicated, groups, replicated_weight):

      sharded      the parameters marked `tensor_model_parallel` (Column / VocabParallel weights and
                   biases, RowParallel weights: each tp rank holds another block),
      replicated   the rest: identical on every tp rank after the backward (sequence parallelism
                   sums the norm weights' partial gradients over the group itself),
      groups       the process-group names to all-reduce (SUM) the squared norm over, in order:
                   "tp" if tp_size > 1, then "pp" if pp_size > 1 (stages hold disjoint layers; cp
                   and dp ranks hold identical gradients after their sync and are not reduced),
      replicated_weight   1 / tp_size: a rank adds sq(sharded) + sq(replicated) / tp, so the tp sum
                   counts every replicated tensor once (a division by a power of two: exact).

    Every rank then holds the same bits, hence the same clip coefficient."""
    if tp_size < 1 or pp_size < 1:
        raise ValueError(f"grad_norm_plan: tp_size={tp_size} pp_size={pp_size}")
    sharded, replicated = [], []
    for p in params:
        (sharded if getattr(p, "tensor_model_parallel", False) else replicated).append(p)
    groups = tuple(name for name, size in (("tp", tp_size), ("pp", pp_size)) if size > 1)
    return sharded, replicated, groups, 1.0 / tp_size


def _listable(*tensors):
    """The layout the multi-tensor launches take: contiguous and 16-byte aligned."""
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors)


def _global_sq(batches):
    """batches: [(multi, [(param, x)])] -- multi: every x is a (param, grad, exp_avg, exp_avg_sq)
    tuple (or a master-weight list's (master, param, grad, exp_avg, exp_avg_sq)) and the batch is one
    multi-tensor list (summed on the descriptor table its AdamW launch uses); else every x is a
    single gradient.  Returns the [1] f32 device scalar holding the squared
    L2 norm over all of them and over the model-parallel grid (grad_norm_plan), or None if there is
    no gradient."""
    m = pgm.current()
    flat = [(p, b, multi, x) for b, (multi, entries) in enumerate(batches) for p, x in entries]
    _, _, groups, w_rep = grad_norm_plan([], m.tp_world_size, m.pp_world_size)
    if w_rep == 1.0:   # nothing is replicated over a group: one pass, every batch as it stands
        parts = [(flat, 1.0)]
    else:
        sharded = {id(p) for p in grad_norm_plan([e[0] for e in flat], m.tp_world_size, m.pp_world_size)[0]}
        parts = [([e for e in flat if id(e[0]) in sharded], 1.0), ([e for e in flat if id(e[0]) not in sharded], w_rep)]
    sq = None
    for part, weight in parts:
        i = 0
        while i < len(part):   # a batch's entries are consecutive
            j = i
            while j < len(part) and part[j][1] == part[i][1]:
                j += 1
            xs = [e[3] for e in part[i:j]]
            sq = K.grad_sqnorm(items=xs if part[i][2] else (), tensors=() if part[i][2] else xs, out=sq,
                               accumulate=sq is not None, weight=weight)
            i = j
    if sq is None:
        return None
    for name in groups:
        dist.all_reduce(sq, op=dist.ReduceOp.SUM, group=getattr(m, f"{name}_group"))
    return sq


class AdamW(torch.optim.Optimizer):
    """max_grad_norm=None: the plain step.  max_grad_norm=M > 0: every step() first takes the global
    L2 norm of all gradients (one f32 pass, every param group, every model-parallel rank: see
    grad_norm_plan) and applies g * min(1, M / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s
    coefficient -- where the AdamW kernel loads the gradient.  The .grad tensors are not modified,
    and no value is read on the host: `last_grad_norm` is a 0-dim f32 DEVICE tensor with the
    pre-clip norm, to be read when the caller synchronises anyway.

    A norm that is inf or NaN skips the update on the device: parameters and both moments stay
    bit-unchanged and a status bit is set, which the next kernels.check_device_status /
    train.read_step_loss raises as HipKernelError.  (Deliberately not torch: clip_grad_norm_ with
    error_if_nonfinite=False would scale by NaN and the step would write NaN into every weight.)
    The host cannot know of the skip without a synchronisation, so state['step'] still counts it.

    master_weights=True (opt-in; the default is the reference's recipe): every bf16 parameter gets an
    f32 `master_param` in its state (from p.float() at the first step) and f32 `exp_avg` /
    `exp_avg_sq`; the step is torch's foreach f32 AdamW on the masters and p = bf16(master), in one
    launch over all such parameters that share a step count and a gradient dtype.  (In bf16 state
    exp_avg_sq * 0.999 rounds back to itself and updates below half an ulp of a weight are lost.)
    Gradients may be bf16 or f32; with max_grad_norm the coefficient multiplies the f32 gradient.
    f32 parameters take the ordinary f32 path.  use_main_grad=True (needs master_weights): a
    parameter with a `main_grad` attribute (DataParallelBucket's f32 accumulator, with
    publish_grad=False the only gradient) is stepped on that tensor and its p.grad is ignored.

    stochastic_rounding=True (opt-in; one or the other, not with master_weights): the state is the
    plain recipe's -- exp_avg / exp_avg_sq in bf16, 6 B per parameter, and a plain-bf16 checkpoint
    loads into such an optimizer and the other way round -- but a bf16 parameter's update is the
    master step's f32 sequence on the widened values, and param, exp_avg and exp_avg_sq are each
    stored with stochastic rounding: E[stored] = the f32 value, so updates below half an ulp
    accumulate in expectation and exp_avg_sq * 0.999 no longer sticks.  Gradients may be bf16 or f32
    (use_main_grad is allowed: an f32 main_grad is consumed as it is); with max_grad_norm the
    coefficient multiplies the f32 gradient.  f32 parameters take the ordinary f32 path.  The random
    bits are Philox4x32-10 on (sr_seed, the parameter's stream id, its step count, the element's
    index, which of the three outputs) and nothing else: sr_seed lives in the param groups, so
    state_dict() carries it, and a parameter's stream id is its position in the flattened
    param_groups (the number state_dict() gives it), so a run resumed from a checkpoint reproduces
    an unbroken one bit for bit.  A non-contiguous parameter is indexed in its logical (row-major)
    order.  dp, cp and tp ranks compute identical bits for replicated parameters; the tp shards of
    one parameter draw from the same stream on every rank, which correlates their rounding noise
    and biases nothing."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 maximize=False, max_grad_norm=None, master_weights=False, use_main_grad=False,
                 stochastic_rounding=False, sr_seed=0):
        if amsgrad or maximize:
            raise ValueError("picotron_amd.optim.AdamW: amsgrad / maximize are not used by picotron (train.py:209)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid AdamW hyper-parameters lr={lr} betas={betas} eps={eps}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"invalid AdamW max_grad_norm={max_grad_norm}: a positive number or None")
        if stochastic_rounding and master_weights:
            raise ValueError("AdamW: stochastic_rounding=True or master_weights=True, one or the other: the masters "
                             "already keep what the rounding would")
        if use_main_grad and not (master_weights or stochastic_rounding):
            raise ValueError("AdamW(use_main_grad=True) needs master_weights=True or stochastic_rounding=True: the "
                             "plain bf16-state step takes the gradient in the parameter's dtype, p.grad")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if stochastic_rounding:
            if int(sr_seed) != sr_seed or not 0 <= int(sr_seed) < 1 << 64:
                raise ValueError(f"invalid AdamW sr_seed={sr_seed}: an unsigned 64-bit integer")
            defaults["sr_seed"] = int(sr_seed)   # in the param groups: state_dict() carries it
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self.master_weights = bool(master_weights)
        self.use_main_grad = bool(use_main_grad)
        self.stochastic_rounding = bool(stochastic_rounding)
        self.sr_seed = int(sr_seed)   # for a group loaded from a checkpoint that has none

    @torch.no_grad()
    def step(self, closure=None):
        """torch.optim.AdamW.step (foreach, decoupled weight decay) on the HIP kernel: the bf16 tensors
        that share a step count go through ONE multi-tensor launch; anything else (f32, unaligned)
        per tensor.  master_weights: the bf16 tensors that share a step count and a gradient dtype
        go through one master-weight launch; stochastic_rounding: likewise, one launch of its own."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is not None:
            self._step_clipped()
            return loss
        for group in self.param_groups:
            for sc, kind, items in self._batches(group):
                _launch(kind, items, sc)
        return loss

    def _grad(self, p):
        """The gradient step() consumes: p.main_grad (DataParallelBucket's averaged accumulator, bf16
        or f32) with use_main_grad where the parameter has one, else p.grad."""
        if self.use_main_grad and getattr(p, "main_grad", None) is not None:
            return p.main_grad
        return p.grad

    def _batches(self, group):
        """[(kernel scalars, kind, items)] of one param group; counts the step.  kind MULTI / SINGLE:
        items are (param, grad, exp_avg, exp_avg_sq), one list launch / one launch each.
        MASTER_MULTI / MASTER_SINGLE (master_weights, bf16 parameters): items are (master_param,
        param, grad, exp_avg, exp_avg_sq); a batch shares the step count and the gradient dtype.
        SR_MULTI / SR_SINGLE (stochastic_rounding, bf16 parameters): items are (param, grad, exp_avg,
        exp_avg_sq, stream id), batched likewise; their scalars carry `seed` and `step` as well."""
        lr, (beta1, beta2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
        batches = {}
        first = 0   # the group's first position in the flattened param_groups
        if self.stochastic_rounding:
            for g in self.param_groups:
                if g is group:
                    break
                first += len(g["params"])
        for pos, p in enumerate(group["params"]):
            grad = self._grad(p)
            if grad is None:
                continue
            if grad.is_sparse:
                raise RuntimeError("AdamW does not support sparse gradients")
            master = self.master_weights and p.dtype == torch.bfloat16
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                if master:
                    st["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                    st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
                else:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if master and "master_param" not in st:   # the first step, or a state loaded without masters
                st["master_param"] = p.detach().float().contiguous()
            st["step"] += 1
            t = st["step"].item()
            if master:
                item = (st["master_param"], p, grad, st["exp_avg"], st["exp_avg_sq"])
                kind = MASTER_MULTI if _listable(*item) else MASTER_SINGLE
                batches.setdefault((t, kind, grad.dtype), []).append(item)
            elif self.stochastic_rounding and p.dtype == torch.bfloat16:
                item = (p, grad, st["exp_avg"], st["exp_avg_sq"])
                kind = SR_MULTI if _listable(*item) else SR_SINGLE
                batches.setdefault((t, kind, grad.dtype), []).append(item + (first + pos,))
            else:
                item = (p, grad, st["exp_avg"], st["exp_avg_sq"])
                multi = p.dtype == grad.dtype == torch.bfloat16 and _listable(*item)
                batches.setdefault((t, MULTI if multi else SINGLE, None), []).append(item)
        out = []
        for (t, kind, _), items in batches.items():
            bc1 = 1 - beta1 ** t
            bc2 = 1 - beta2 ** t
            sc = dict(decay=1 - lr * wd, w1=1 - beta1, beta2=beta2, c2=1 - beta2, bc2_sqrt=bc2 ** 0.5, eps=eps,
                      step_size=(lr / bc1) * -1)
            if kind in (SR_MULTI, SR_SINGLE):
                sc.update(seed=group.get("sr_seed", self.sr_seed), step=int(t))
            out.append((sc, kind, items))
        return out

    def _step_clipped(self):
        work, norm_batches = self._clip_work()
        sq = _global_sq(norm_batches)
        if sq is None:   # no gradients at all
            return
        self._launch_clipped(work, sq, self.max_grad_norm)

    def _clip_work(self):
        """(the step's batches, what _global_sq takes for their gradients); counts the step.  Split
        from the launch so that a caller holding further parameters (MuonAdamW) can take ONE norm
        over all of them and hand it to _launch_clipped."""
        work = [b for group in self.param_groups for b in self._batches(group)]
        norm_batches = []
        for _, kind, items in work:   # (param, what grad_sqnorm takes for it): see _global_sq
            _, is_list, ip, ig = _KINDS[kind]
            if is_list:
                norm_batches.append((True, [(it[ip], it) for it in items]))
            else:   # the gradient as the step will take it (_master_single, _sr_single)
                dense = kind in (MASTER_SINGLE, SR_SINGLE)
                norm_batches.append((False, [(it[ip], it[ig].contiguous() if dense else it[ig]) for it in items]))
        return work, norm_batches

    def _launch_clipped(self, work, sq, max_norm, status=None):
        """The clipped launches of _clip_work's batches on the squared norm sq.  status: the caller's
        status word, which the caller then posts itself."""
        self.last_grad_norm = sq.sqrt().reshape(())
        own = status is None
        if own:
            status = K.status_word(sq.device)   # one word, posted once: see kernels._clip_status
        for sc, kind, items in work:
            _launch(kind, items, sc, clip=(sq, max_norm, status))
        if own:
            K._status_posted(sq.device)

    @torch.no_grad()
    def sync_master_from_params(self):
        """Re-read every master weight from its bf16 parameter: for a caller that overwrites weights
        (loads a checkpoint into the model, copies from another rank) after the first step()."""
        for st_p, st in self.state.items():
            if isinstance(st, dict) and "master_param" in st:
                st["master_param"].copy_(st_p.detach().reshape(st["master_param"].shape))

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict, which casts every floating-point state tensor to the
        parameter's dtype -- with master_weights the f32 `master_param`, `exp_avg` and `exp_avg_sq`
        of a bf16 parameter are put back from the saved dict afterwards, bit for bit.  A bf16-state
        dict (master_weights=False) loads into master_weights=True: the moments are widened and the
        masters are taken from the parameters at the next step.  The other direction is refused.
        stochastic_rounding keeps the plain recipe's bf16 state: it loads a plain checkpoint and a
        plain optimizer loads its, and f32 master state is refused as without it."""
        saved = list(itertools.chain.from_iterable(g["params"] for g in state_dict["param_groups"]))
        mine = list(itertools.chain.from_iterable(g["params"] for g in self.param_groups))
        pairs = [(state_dict["state"][k], p) for k, p in zip(saved, mine) if k in state_dict["state"]]
        if not self.master_weights:
            for s, p in pairs:
                f32 = [k for k in ("exp_avg", "exp_avg_sq") if torch.is_tensor(s.get(k)) and s[k].dtype == torch.float32]
                if p.dtype == torch.bfloat16 and ("master_param" in s or f32):
                    raise ValueError("AdamW.load_state_dict: the state holds f32 master weights / moments of a bf16 "
                                     "parameter (saved with master_weights=True); this optimizer has "
                                     "master_weights=False and would round them to bf16 -- construct it with "
                                     "master_weights=True")
        super().load_state_dict(state_dict)
        if self.master_weights or self.stochastic_rounding:
            for s, p in pairs:
                if torch.is_tensor(self.state[p].get("step")):
                    # torch hands the saved `step` tensor through as it is; a live optimizer's
                    # state_dict() loaded here would share (and double-count) it
                    self.state[p]["step"] = self.state[p]["step"].clone()
                if not self.master_weights or p.dtype != torch.bfloat16:
                    continue
                for k in ("master_param", "exp_avg", "exp_avg_sq"):
                    if torch.is_tensor(s.get(k)):
                        self.state[p][k] = s[k].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()


MULTI, SINGLE, MASTER_MULTI, MASTER_SINGLE = "multi", "single", "master_multi", "master_single"
SR_MULTI, SR_SINGLE = "sr_multi", "sr_single"
# kind -> (kernels.* step function, + "_clip" for the clipped one; list launch?; index of param, of grad in an item)
_KINDS = {MULTI: ("adamw_step_multi", True, 0, 1), SINGLE: ("adamw_step", False, 0, 1),
          MASTER_MULTI: ("adamw_master_step_multi", True, 1, 2), MASTER_SINGLE: ("adamw_master_step", False, 1, 2),
          SR_MULTI: ("adamw_sr_step_multi", True, 0, 1), SR_SINGLE: ("adamw_sr_step", False, 0, 1)}


def _launch(kind, items, sc, clip=None):
    """One batch of AdamW._batches; clip = (sq, max_norm, status word): the clipped kernels."""
    name, is_list, _, _ = _KINDS[kind]
    fn = getattr(K, name if clip is None else name + "_clip")
    args, kw = ((), sc) if clip is None else (clip[:2], dict(sc, status=clip[2]))
    if is_list:
        return fn(items, *args, **kw)
    for it in items:
        if kind == MASTER_SINGLE:
            _master_single(fn, it, *args, **kw)
        elif kind == SR_SINGLE:
            _sr_single(fn, it, *args, **kw)
        else:
            fn(*it, *args, **kw)


def _master_single(fn, item, *args, **kw):
    """One master-weight entry the list launch does not take: an unaligned view goes to the
    single-tensor kernel as it is; a non-contiguous parameter or gradient through a dense copy."""
    w, p, g, m, v = item
    if p.is_contiguous():
        fn(w, p, g.contiguous(), m, v, *args, **kw)
    else:
        dense = p.detach().contiguous()   # the current weights: a skipped (non-finite) step leaves them
        fn(w, dense, g.contiguous(), m, v, *args, **kw)
        p.copy_(dense)


def _sr_single(fn, item, *args, **kw):
    """One stochastic-rounding entry the list launch does not take: an unaligned view goes to the
    single-tensor kernel as it is; a non-contiguous parameter, moment or gradient through a dense
    copy (the element index of the random bits is the logical, row-major one)."""
    p, g, m, v, stream = item
    dense = [t if t.is_contiguous() else t.detach().contiguous() for t in (p, m, v)]
    fn(dense[0], g.contiguous(), dense[1], dense[2], stream, *args, **kw)
    for t, d in zip((p, m, v), dense):
        if d is not t:   # the current values: a skipped (non-finite) step left them
            t.copy_(d)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for a reference-style train.py (in front of optimizer.step()):
    the global L2 norm in f32 over every gradient and every tensor- / pipeline-parallel rank
    (grad_norm_plan), then grad = r(grad * min(1, max_norm / (norm + 1e-6))) in place -- all on the
    device.  Returns the total norm as a 0-dim f32 device tensor.  L2 only.  A non-finite norm
    leaves the gradients alone and is raised by the next kernels.check_device_status, whatever
    error_if_nonfinite says (checking it here would be a host synchronisation)."""
    if float(norm_type) != 2.0:
        raise ValueError(f"picotron_amd.optim.clip_grad_norm_: only the L2 norm (norm_type=2), got {norm_type}")
    if not float(max_norm) > 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm={max_norm} must be positive")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    listed = {id(p) for p in params if p.grad.dtype == torch.bfloat16 and _listable(p.grad)}
    multi = [(p, (p.grad,) * 4) for p in params if id(p) in listed]
    single = [(p, p.grad) for p in params if id(p) not in listed]
    sq = _global_sq([(True, multi), (False, single)])
    status = K.status_word(sq.device)
    if multi:
        K.grad_scale_multi([x for _, x in multi], sq, max_norm, status=status)
    for _, g in single:
        K.grad_scale(g, sq, max_norm, status=status)
    K._status_posted(sq.device)
    return sq.sqrt().reshape(())


# ------------------------------------------------------------------------------------ Muon
_MUON_MATRICES = ("attention.q_proj.weight", "attention.k_proj.weight", "attention.v_proj.weight",
                  "attention.out_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
_MUON_EXPERT_MATRICES = ("gate_proj.weight", "up_proj.weight", "down_proj.weight")   # under mlp.experts.{e}.


def split_muon_params(model):
    """(matrices, rest) of a Llama: `matrices` the decoder layers' q / k / v / out / gate / up / down
    projection weights (what Muon orthogonalises; of a mixture-of-experts layer every expert's
    mlp.experts.{e}.gate / up / down), `rest` everything else -- the embedding, final_proj, every norm
    weight (QK-norm's included), an MoE layer's mlp.router.weight and the biases -- for AdamW.  By
    parameter name, in named_parameters() order."""
    matrices, rest = [], []
    for name, p in model.named_parameters():
        expert = ".mlp.experts." in name and name.endswith(_MUON_EXPERT_MATRICES)
        hidden = "decoder_layers." in name and (name.endswith(_MUON_MATRICES) or expert) and p.dim() == 2
        (matrices if hidden else rest).append(p)
    return matrices, rest


class Muon(torch.optim.Optimizer):
    """torch.optim.Muon on the HIP kernels: the same constructor, defaults, param_groups keys and
    state key (`momentum_buffer`), so a state_dict of one loads into the other.  Per 2-D bf16
    parameter p [R, C] (csrc/muon.hip, kernels.muon_newton_schulz):

        buf = lerp(buf, g, 1 - momentum); u = bf16(lerp(g, buf, momentum) | buf)
        X0 = bf16(u / max(||u||_F, eps))          the norm in f32 on the device, never on the host
        ns_steps x:  A = bf16(X X^T); S = f32(A A); P' = bf16(a I + b A + c S); X = bf16(P' X)
        p = bf16(p (1 - lr wd)); p = bf16(p - lr_adj X)

    The momentum, scale and apply kernels each run once over the whole list; the GEMMs of
    same-shaped matrices run four to a launch.  Nothing synchronises with the host, nothing is
    atomic: data-, context- and pipeline-parallel replicas compute identical bits.

    use_main_grad=True (the added argument): a parameter with a `main_grad` attribute
    (DataParallelBucket's accumulator, bf16 or f32) is stepped on that tensor and its p.grad is
    ignored; the momentum buffer has the gradient's dtype.

    Refused: parameters that are not 2-D or not floating point (ValueError, as torch); f32
    parameters (NotImplementedError: the kernels store bf16); a parameter marked
    `tensor_model_parallel` while tp > 1 (NotImplementedError: Newton-Schulz needs the whole
    matrix, and a rank holds a block of it)."""

    def __init__(self, params, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None,
                 use_main_grad=False):
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"momentum should be >= 0 but is: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        if adjust_lr_fn is not None and adjust_lr_fn not in ("original", "match_rms_adamw"):
            raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
        if len(ns_coefficients) != 3:
            raise ValueError("Coefficients must be a tuple of exactly 3 values")
        if not 0 <= int(ns_steps) < 100:
            raise ValueError("Number of steps must be less than 100 for computational efficiency")
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                        ns_coefficients=ns_coefficients, eps=eps, ns_steps=ns_steps, adjust_lr_fn=adjust_lr_fn)
        super().__init__(params, defaults)
        tp = pgm.current().tp_world_size
        for group in self.param_groups:
            for p in group["params"]:
                if p.ndim != 2:
                    raise ValueError(f"Muon only supports 2D parameters whereas we found a parameter with size: {p.size()}")
                if p.dtype == torch.float32:
                    raise NotImplementedError("picotron_amd.optim.Muon: f32 parameters are not supported (the kernels "
                                              "store bf16); keep them on AdamW")
                if p.dtype != torch.bfloat16:
                    raise ValueError(f"picotron_amd.optim.Muon: bf16 parameters only, got {p.dtype}")
                if tp > 1 and getattr(p, "tensor_model_parallel", False):
                    raise NotImplementedError("picotron_amd.optim.Muon: a tensor-parallel shard (tp > 1): Newton-Schulz "
                                              "needs the whole matrix")
        self.use_main_grad = bool(use_main_grad)
        self._x = {}   # parameter -> its workspace image (X0 / O); not optimizer state

    def _grad(self, p):
        if self.use_main_grad and getattr(p, "main_grad", None) is not None:
            return p.main_grad
        return p.grad

    def _work(self):
        """[(group, items, fix)] -- one list per param group and gradient dtype, items as kernels.muon_*
        take them; fix: (parameter, dense copy) pairs to copy back after the apply (a parameter whose
        column stride is not 1)."""
        work = []
        for group in self.param_groups:
            lists = {}
            for p in group["params"]:
                g = self._grad(p)
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Muon does not support sparse gradients")
                if g.dtype not in (torch.bfloat16, torch.float32):
                    raise ValueError(f"picotron_amd.optim.Muon: bf16 or f32 gradients, got {g.dtype}")
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros(p.shape, dtype=g.dtype, device=p.device)
                buf = st["momentum_buffer"]
                if buf.dtype != g.dtype or buf.stride(1) != 1:   # a loaded state in another dtype
                    buf = st["momentum_buffer"] = buf.to(g.dtype).contiguous()
                x = self._x.get(p)
                if x is None:
                    x = self._x[p] = K.muon_x_workspace(p.shape, p.device)
                pd = p if p.stride(1) == 1 and p.stride(0) >= p.shape[1] else p.detach().contiguous()
                gd = g if g.stride(1) == 1 and g.stride(0) >= g.shape[1] else g.contiguous()
                items, fix = lists.setdefault(g.dtype, ([], []))
                items.append((pd, gd, buf, x, K.muon_lr_ratio(group["adjust_lr_fn"], p.shape)))
                if pd is not p:
                    fix.append((p, pd))
            work.extend((group, items, fix) for items, fix in lists.values())
        return work

    @torch.no_grad()
    def step(self, closure=None, stages=None):
        """stages: a list that receives, per launched list (param group x gradient dtype), a dict of
        the step's intermediates for the conformance tests -- `params`, `sq` and what
        kernels.muon_newton_schulz(stages=) records."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(self._work(), None, stages)
        return loss

    def _run(self, work, clip, stages=None):
        """clip = (global sq, max_norm, status word) from MuonAdamW, or None."""
        for group, items, fix in work:
            mu, nes = group["momentum"], group["nesterov"]
            rec = None if stages is None else {"params": [it[0] for it in items]}
            sq = K.muon_momentum(items, mu, nes, clip=clip)
            K.muon_scale(items, sq, mu, nes, group["eps"], clip=clip)
            K.muon_newton_schulz([it[3] for it in items], group["ns_coefficients"], group["ns_steps"], stages=rec)
            K.muon_apply(items, group["lr"], group["weight_decay"], clip=clip)
            if rec is not None:
                rec["sq"] = sq
                stages.append(rec)
            for p, dense in fix:
                p.copy_(dense)

    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict, which casts every floating-point state tensor to the
        parameter's dtype -- an f32 momentum buffer (use_main_grad with f32 accumulators) is put back
        from the saved dict afterwards, bit for bit."""
        saved = list(itertools.chain.from_iterable(g["params"] for g in state_dict["param_groups"]))
        mine = list(itertools.chain.from_iterable(g["params"] for g in self.param_groups))
        super().load_state_dict(state_dict)
        for k, p in zip(saved, mine):
            buf = state_dict["state"].get(k, {}).get("momentum_buffer")
            if torch.is_tensor(buf) and buf.dtype == torch.float32:
                self.state[p]["momentum_buffer"] = buf.detach().to(device=p.device, dtype=torch.float32, copy=True)

    def _norm_batches(self, work):
        """What _global_sq takes for the gradients of _work()'s lists."""
        out = []
        for _, items, _ in work:
            listed = [it for it in items if it[1].dtype == torch.bfloat16 and _listable(it[1])]
            ids = {id(it) for it in listed}
            out.append((True, [(it[0], (it[1],) * 4) for it in listed]))
            out.append((False, [(it[0], it[1].contiguous()) for it in items if id(it) not in ids]))
        return [b for b in out if b[1]]


class MuonAdamW:
    """Muon for the hidden matrices and AdamW for the rest, as one optimizer object: step / zero_grad
    / state_dict / load_state_dict, and `param_groups` = Muon's followed by AdamW's (the same dict
    objects, so a schedule that writes group["lr"] drives both).  Not a torch.optim.Optimizer:
    torch.optim.lr_scheduler classes take `.muon` and `.adamw`, one scheduler each, and a new param
    group is added to the inner optimizer that is to own it (`param_groups` is rebuilt from the two on
    every access).

    MuonAdamW(model) splits with split_muon_params; MuonAdamW((matrices, rest)) takes a split.
    muon= / adamw= are the keyword arguments of optim.Muon / optim.AdamW (every AdamW form stays
    available: master_weights, stochastic_rounding, use_main_grad).  max_grad_norm=M: ONE global L2
    norm over the gradients of both parts (and the model-parallel grid, grad_norm_plan); the same
    device scalar feeds AdamW's clipped launches and Muon's clipped momentum kernel, so the whole
    model is scaled by one coefficient; a non-finite norm skips the whole step on the device."""

    def __init__(self, model_or_split, muon=None, adamw=None, max_grad_norm=None):
        if isinstance(model_or_split, torch.nn.Module):
            matrices, rest = split_muon_params(model_or_split)
        else:
            matrices, rest = (list(x) for x in model_or_split)
        adamw = dict(adamw or {})
        if "max_grad_norm" in adamw:
            raise ValueError("MuonAdamW: max_grad_norm belongs to MuonAdamW itself (one norm over both parts)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"invalid MuonAdamW max_grad_norm={max_grad_norm}: a positive number or None")
        self.muon = Muon(matrices, **dict(muon or {}))
        self.adamw = AdamW(rest, **adamw)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self.last_grad_sq = None   # the [1] f32 device scalar both parts took their coefficient from

    @property
    def param_groups(self):
        return self.muon.param_groups + self.adamw.param_groups

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is None:
            self.muon.step()
            self.adamw.step()
            return loss
        mwork = self.muon._work()
        awork, abatches = self.adamw._clip_work()
        sq = _global_sq(self.muon._norm_batches(mwork) + abatches)
        if sq is None:   # no gradients at all
            return loss
        self.last_grad_sq = sq
        self.last_grad_norm = sq.sqrt().reshape(())
        status = K.status_word(sq.device)   # one word for the whole step, posted once
        self.muon._run(mwork, (sq, self.max_grad_norm, status))
        self.adamw._launch_clipped(awork, sq, self.max_grad_norm, status=status)
        K._status_posted(sq.device)
        return loss

    def zero_grad(self, set_to_none=True):
        self.muon.zero_grad(set_to_none=set_to_none)
        self.adamw.zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        return {"muon": self.muon.state_dict(), "adamw": self.adamw.state_dict()}

    def load_state_dict(self, state_dict):
        self.muon.load_state_dict(state_dict["muon"])
        self.adamw.load_state_dict(state_dict["adamw"])
