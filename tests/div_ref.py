"""fp64 reference of the token-level KD divergences (kdstep.h KD_LOSS_FKL / RKL / JSD).

Inputs are bf16-representable logits (the kernel sees exactly these values).  Per row (one
(b, l) position), p = softmax(t[:V_s] / T), q = softmax(s / T), everything from log_softmax
(log m of the JSD mixture from logaddexp), so no log of an underflowed probability:

    fkl  D = sum_v p (log p - log q)
    rkl  D = sum_v q (log q - log p)
    jsd  D = sum_v [beta p (log p - log m) + (1 - beta) q (log q - log m)],  m = beta p + (1 - beta) q

KD term = T^2 / R * sum of D over the row set: "all" = every row (R = B L), "targets" = the rows
whose shifted label is a CE target (R = their number; R = 0 gives 0).  The student CE is the
causal-LM loss (shift by one, ignore -100, mean over the targets).  Gradients w.r.t. the
student logits come from autograd.  A_row = sum_v |summand_v| is the uncancelled magnitude of a
row's sum: what an absolute error bound on the KD term is scaled by.
"""
import torch

DIVERGENCES = ("fkl", "rkl", "jsd")


def row_summands(t, s, kind, T=1.0, beta=0.5):
    """[rows, V_s] fp64 summands of D for teacher / student logits [..., V_t] / [..., V_s]."""
    V = s.shape[-1]
    lp = torch.log_softmax(t[..., :V].double() / T, -1)
    lq = torch.log_softmax(s.double() / T, -1)
    if kind == "fkl":
        return lp.exp() * (lp - lq)
    if kind == "rkl":
        return lq.exp() * (lq - lp)
    if kind == "jsd":
        b = torch.tensor(float(beta), dtype=torch.float64, device=s.device)
        lm = torch.logaddexp(lp + b.log(), lq + (1 - b).log())
        return b * lp.exp() * (lp - lm) + (1 - b) * lq.exp() * (lq - lm)
    raise ValueError(kind)


def target_rows(labels, V):
    """[B, L] bool: the row's shifted label is a CE target (RowStats.valid)."""
    nxt = torch.full_like(labels, -100)
    nxt[:, :-1] = labels[:, 1:]
    return (nxt >= 0) & (nxt < V), nxt


def div_ref(t, s, labels, kind, T=1.0, beta=0.5, rows="all", kd_weight=1.0, ce_weight=1.0, want_grad=True):
    """dict(kd, ce, total: 0-d fp64; A: [B*L] fp64; valid: [B*L] bool; grad, grad_kd: [B*L, V_s] fp64
    d total / d s and d (kd_weight kd) / d s, or None).  ce is NaN without targets (the mean of nothing),
    as the kernel's; the gradients then hold the KD part alone."""
    B, L, V = s.shape
    sd = s.detach().double().requires_grad_(want_grad)
    valid, nxt = target_rows(labels, V)
    with torch.set_grad_enabled(want_grad):
        summ = row_summands(t, sd, kind, T, beta).reshape(B * L, V)
        D = summ.sum(-1)
        if rows == "all":
            kd = D.mean() * T * T
            A_sel = torch.ones(B * L, dtype=torch.bool, device=s.device)
        elif rows == "targets":
            A_sel = valid.reshape(-1)
            n = int(A_sel.sum())
            kd = (D[A_sel].sum() / n if n else D.sum() * 0.0) * T * T
        else:
            raise ValueError(rows)
        lq1 = torch.log_softmax(sd, -1).reshape(B * L, V)
        vr = valid.reshape(-1)
        nv = int(vr.sum())
        ce_sum = -lq1[vr].gather(1, nxt.reshape(-1)[vr][:, None]).sum()
        ce = ce_sum / nv if nv else ce_sum * float("nan")
    out = dict(kd=kd.detach(), ce=ce.detach(), total=(kd_weight * kd + ce_weight * ce).detach(),
               A=summ.detach().abs().sum(-1), valid=vr, rows_sel=A_sel, grad=None, grad_kd=None)
    if want_grad:
        gk, = torch.autograd.grad(kd_weight * kd, sd, retain_graph=True)
        g = gk
        if nv and ce_weight != 0.0:
            gc, = torch.autograd.grad(ce_weight * ce, sd)
            g = gk + gc
        out["grad_kd"], out["grad"] = gk.reshape(B * L, V), g.reshape(B * L, V)
    return out


def kd_bound(ref, T):
    """|got - ref| bound of the KD term: 1e-4 x the mean over the row set of A_row x T^2 (a relative
    1e-4 taken on the uncancelled sum; the term itself may be exactly 0)."""
    sel = ref["rows_sel"]
    a = float(ref["A"][sel].mean()) if bool(sel.any()) else 0.0
    return 1e-4 * a * T * T
