"""Float64 restatement of the Diffusion-DPO loss (include/sdt.h "DPO LOSS") from (pred, ref_pred, target, beta), and the fp32 / bf16
chains that lead from one published output of sdt_dpo_loss_fwd_bwd to the next.

B = 2P samples, sample 2i the preferred image of pair i and 2i+1 the rejected one.  pred / ref_pred: (B, h, w, C) (the valid channels
of the NHWC tensors), target: (B, C, h, w).  With m_b, r_b the per-sample mean squared errors of the trained and the reference pass:
    z_i = -beta/2 * ((m_w - m_l) - (r_w - r_l)),   loss = mean_i -logsigmoid(z_i),   s_i = sigmoid(-z_i),
    d loss / d pred[b] = coef_b * (target - pred) / (P*C*h*w),   coef_w = -beta * s,  coef_l = +beta * s."""
import numpy as np
import torch

F32 = np.float32


def neg_logsigmoid(z):
    """-log(sigmoid(z)) in the form that cannot overflow: max(-z, 0) + log1p(exp(-|z|))."""
    z = np.asarray(z, dtype=np.float64)
    return np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid_neg(z):
    """sigmoid(-z) from the exponential of a non-positive argument: e / (1 + e) for z >= 0, 1 / (1 + e) for z < 0, e = exp(-|z|)."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def sample_sq_sums(x, target):
    """a_b = sum_{c,p} fl(fl(target - x)^2) over each sample, accumulated in float64 from the fp32 element chain: (B,) float64."""
    x = np.asarray(x, dtype=F32)
    t = np.asarray(target, dtype=F32).transpose(0, 2, 3, 1)
    d = (t - x).astype(F32)
    return (d * d).astype(F32).astype(np.float64).reshape(d.shape[0], -1).sum(1)


def publish_mse(a64, n):
    """m_b = fl(fl(a_b) * fl(1/n)) as the kernel publishes it (fp32); a_b is exact when the inputs make every partial sum representable."""
    return (a64.astype(F32) * (F32(1.0) / F32(n))).astype(F32)


def pairs(m32, r32, beta):
    """Everything per pair, in float64 from the published fp32 sample_mse rows: dict(z, logits, pair_loss, s, coef); logits is the one
    fp32 rounding of z (bit-exact: only +, -, x in double), pair_loss / coef are float64 (the device's exp / log1p are not correctly
    rounded: compare within 1 fp32 ulp)."""
    m, r = np.asarray(m32, dtype=F32).astype(np.float64), np.asarray(r32, dtype=F32).astype(np.float64)
    b = float(F32(beta))
    delta = (m[0::2] - m[1::2]) - (r[0::2] - r[1::2])
    z = (-0.5 * b) * delta
    s = sigmoid_neg(z)
    coef = np.empty(m.shape[0], dtype=np.float64)
    coef[0::2], coef[1::2] = -b * s, b * s
    return dict(z=z, logits=z.astype(F32), pair_loss=neg_logsigmoid(z), s=s, coef=coef)


def loss_chain(pair_loss32):
    """loss = fl(T * fl(1/P)), T the published pair losses added in pair order in fp32."""
    t = F32(0.0)
    for v in np.asarray(pair_loss32, dtype=F32):
        t = F32(t + v)
    return F32(t * (F32(1.0) / F32(len(pair_loss32))))


def dpred_chain(coef32, pred, target):
    """bf16_rne(fl(fl(coef_b * fl(target - pred)) * inv_count)), inv_count = fl(1 / fl(P*C*h*w)), from the published coef: a torch
    bfloat16 tensor (B, h, w, C)."""
    x = np.asarray(pred, dtype=F32)
    t = np.asarray(target, dtype=F32).transpose(0, 2, 3, 1)
    B, h, w, C = x.shape
    inv = F32(1.0) / F32((B // 2) * C * h * w)
    d = (t - x).astype(F32)
    g = (np.asarray(coef32, dtype=F32).reshape(B, 1, 1, 1) * d).astype(F32)
    return torch.from_numpy((g * inv).astype(F32)).to(torch.bfloat16)


def reference(pred, ref_pred, target, beta):
    """The whole loss in float64 from the fp32 / bf16-valued inputs, nothing rounded in between: dict(loss, logits, pair_loss, coef,
    model_mse, ref_mse, dpred)."""
    x, y = np.asarray(pred, dtype=np.float64), np.asarray(ref_pred, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64).transpose(0, 2, 3, 1)
    B, h, w, C = x.shape
    m = ((t - x) ** 2).reshape(B, -1).mean(1)
    r = ((t - y) ** 2).reshape(B, -1).mean(1)
    z = -0.5 * float(beta) * ((m[0::2] - m[1::2]) - (r[0::2] - r[1::2]))
    pl, s = neg_logsigmoid(z), sigmoid_neg(z)
    coef = np.empty(B)
    coef[0::2], coef[1::2] = -float(beta) * s, float(beta) * s
    dpred = coef.reshape(B, 1, 1, 1) * (t - x) / ((B // 2) * C * h * w)
    return dict(loss=pl.mean(), logits=z, pair_loss=pl, coef=coef, model_mse=m, ref_mse=r, dpred=dpred)


def loss_torch(pred, ref_pred, target, beta):
    """The same loss as a differentiable torch expression (float64 tensors, pred (B,h,w,C), target (B,C,h,w)): what autograd is checked
    against the closed form with."""
    t = target.permute(0, 2, 3, 1)
    m = ((t - pred) ** 2).flatten(1).mean(1)
    r = ((t - ref_pred) ** 2).flatten(1).mean(1)
    z = -0.5 * beta * ((m[0::2] - m[1::2]) - (r[0::2] - r[1::2]))
    return -torch.nn.functional.logsigmoid(z).mean()
