"""The sigmoid router (kernels.moe_route_sigmoid / moe_route_sigmoid_bwd) in float64, torch ops only:
    s = sigmoid(stored bf16 logit), key = s + bias; G contiguous groups, a group's score = its two largest
    keys' sum, the Kg best groups stay (ties to the lower group); idx = the k largest keys inside them
    (ties to the lower expert, best first); gate = scale s[idx] (/ (their sum + 1e-20) under norm);
    aux = E sum_e (counts_e / (T k)) mean_t (s / sum_e s)[t, e].
margin[t]: the smaller of the gaps between the Kg-th and (Kg + 1)-th group score and between the k-th and
(k + 1)-th kept key; a token under MARGIN may legitimately choose differently in f32 and is not compared.
A gap of exactly 0 is no such case: equal stored logits give equal scores in any precision (bf16 logits
repeat within a row), the index decides, and the gap that counts is the one to the next smaller value."""
import torch

F64, I32 = torch.float64, torch.int32
MARGIN, MAX_EXCLUDED = 1e-5, 0.01


def inputs(T, E, k, seed, ldl=None):
    """(logits bf16 [T, E] (a view of [T, ldl]), bias f32 [E], dgate f32 [T, k], d_aux f32 [1]) of one seed."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, ldl or E, generator=g) * 2).to(torch.bfloat16)[:, :E]
    return logits, torch.randn(E, generator=g) * 0.1, torch.randn(T, k, generator=g), torch.randn(1, generator=g)


def _gap(sorted_desc, n):
    """The n-th value minus the largest strictly smaller one behind it (inf: none)."""
    gap = sorted_desc[:, n - 1:n] - sorted_desc[:, n:]
    return gap.masked_fill(gap == 0, float("inf")).min(1).values


def ref_route(logits, bias, k, G, Kg, norm, scale, idx=None):
    """(idx, gate, s, counts, aux, margin); idx given: gate, counts and aux of that selection."""
    T, E = logits.shape
    s = torch.sigmoid(logits.to(F64))
    cand = s + (bias.to(F64) if bias is not None else 0.0)
    margin = torch.full((T,), float("inf"), dtype=F64)
    if G > 1:
        score = cand.view(T, G, E // G).topk(2, dim=2).values.sum(2)
        order = torch.sort(score, dim=1, descending=True, stable=True)
        if Kg < G:
            margin = _gap(order.values, Kg)
        kept = torch.zeros(T, G, dtype=torch.bool).scatter_(1, order.indices[:, :Kg], True)
        cand = cand.masked_fill(~kept.repeat_interleave(E // G, dim=1), float("-inf"))
    order = torch.sort(cand, dim=1, descending=True, stable=True)
    if k < E:
        margin = torch.minimum(margin, _gap(order.values, k))
    if idx is None:
        idx = order.indices[:, :k].to(I32)
    sel = s.gather(1, idx.long())
    gate = scale * (sel / (sel.sum(1, keepdim=True) + 1e-20) if norm else sel)
    counts = torch.bincount(idx.reshape(-1).long(), minlength=E).to(I32)
    aux = E * ((counts.to(F64) / (T * k)) * (s / s.sum(1, keepdim=True)).mean(0)).sum()
    return idx, gate, s, counts, aux.reshape(1), margin


def ref_route_bwd(logits, idx, dgate, d_aux, norm, scale, tol):
    """(dlogits float64 [T, E], allowance float64 [T, E]) with idx and counts held fixed.  The allowance is
    tests/_moe_ref.route_bwd_allowance's reasoning on this router's formulas: the kernel reads scores that
    carry a relative error tol, so every ds[t, e] is off by at most 4 tol m[t, e], m the sum of the
    magnitudes that meet in it; dlogit = ds s (1 - s) adds the error of s (tol) and of 1 - s (tol s,
    absolute): at most tol m s (5 (1 - s) + s) <= 8 tol m s."""
    T, E = logits.shape
    k = idx.shape[1]
    s = torch.sigmoid(logits.to(F64))
    sel, dg = s.gather(1, idx.long()), dgate.to(F64)
    if norm:
        S = sel.sum(1, keepdim=True) + 1e-20
        gate = scale * sel / S
        dsel, msel = (scale * dg - (dg * gate).sum(1, keepdim=True)) / S, (scale * dg.abs() + (dg.abs() * gate).sum(1, keepdim=True)) / S
    else:
        dsel, msel = scale * dg, scale * dg.abs()
    dq = float(d_aux) * E * (torch.bincount(idx.reshape(-1).long(), minlength=E).to(F64) / (T * k)) / T
    tot = s.sum(1, keepdim=True)
    q = s / tot
    ds = ((dq - (q * dq).sum(1, keepdim=True)) / tot).scatter_add(1, idx.long(), dsel)
    m = ((dq.abs() + (q * dq.abs()).sum(1, keepdim=True)) / tot).scatter_add(1, idx.long(), msel)
    return ds * s * (1 - s), 8 * tol * m * s
