"""NumPy float32 restatement of the samplers' new paths (test infrastructure, independent of the package's schedulers.py):
diffusers 0.21.4 FlaxDPMSolverMultistepScheduler with algorithm_type "dpmsolver++", solver_type "midpoint" (tables,
convert_model_output, dpm_solver_first_order_update, multistep_dpm_solver_second_order_update) and diffusers'
rescale_noise_cfg.  Every table and every operation stays float32, in the order the formulas are written."""
import numpy as np

F32 = np.float32


def tables(alphas_cumprod):
    ac = np.asarray(alphas_cumprod, dtype=F32)
    alpha = np.sqrt(ac).astype(F32)
    sigma = np.sqrt(F32(1) - ac).astype(F32)
    with np.errstate(divide="ignore"):
        lam = (np.log(alpha) - np.log(sigma)).astype(F32)  # -inf where ac == 0
    return alpha, sigma, lam


def to_x0(prediction_type, m, x, alpha_s, sigma_s):
    if prediction_type == "epsilon":
        return (x - sigma_s * m) / alpha_s
    if prediction_type == "sample":
        return m
    return alpha_s * x - sigma_s * m


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale):
    """diffusers' rescale_noise_cfg (torch float32, std over every axis but the batch)."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


def rescale_factors(un, tx, guidance_scale, guidance_rescale):
    """f_b = phi * std(tx_b) / std(cfg_b) + (1 - phi) in float64 from float32 cfg = un + g (tx - un); (B, ...) tensors."""
    cfg = (un + float(guidance_scale) * (tx - un)).double()
    dims = list(range(1, tx.ndim))
    return guidance_rescale * tx.double().std(dim=dims) / cfg.std(dim=dims) + (1 - guidance_rescale)


def guided(un, tx, guidance_scale, guidance_rescale):
    """cfg = un + g (tx - un), rescaled as the HIP path does it: cfg * f_b, f_b rounded to float32 (torch float32 tensors)."""
    cfg = un + float(guidance_scale) * (tx - un)
    if guidance_rescale == 0.0:
        return cfg
    f = rescale_factors(un, tx, guidance_scale, guidance_rescale).float()
    return cfg * f.view(-1, *([1] * (cfg.ndim - 1)))


class DPMSolverPP:
    """Step i: s0 = timesteps[i] -> t = timesteps[i+1] (0 after the last).  step() takes the guided model output m and the
    sample x (float32 arrays) and returns x_t; the x0 of the previous step is kept here."""

    def __init__(self, alphas_cumprod, timesteps, prediction_type, solver_order=2, lower_order_final=True):
        self.alpha, self.sigma, self.lam = tables(alphas_cumprod)
        self.ts = [int(t) for t in timesteps]
        self.ptype, self.order, self.lower_order_final = prediction_type, solver_order, lower_order_final
        self.x0_prev = None

    def first_order(self, i):
        n = len(self.ts)
        return self.order == 1 or i == 0 or (self.lower_order_final and i == n - 1 and n < 15)

    def terms(self, i):
        """The scalars of step i: s0, t, sigma_t / sigma_s0, alpha_t (e^-h - 1), and 1 / r0 (None at a first-order step)."""
        n = len(self.ts)
        s0 = self.ts[i]
        t = self.ts[i + 1] if i + 1 < n else 0
        a, s, lam = self.alpha, self.sigma, self.lam
        h = lam[t] - lam[s0]
        ah = a[t] * (np.exp(-h) - F32(1))
        inv_r0 = None
        if not self.first_order(i):
            h0 = lam[s0] - lam[self.ts[i - 1]]
            inv_r0 = F32(1) / (h0 / h)
        return s0, t, s[t] / s[s0], ah, inv_r0

    def step(self, i, m, x):
        m, x = np.asarray(m, dtype=F32), np.asarray(x, dtype=F32)
        s0, t, ratio, ah, inv_r0 = self.terms(i)
        x0 = to_x0(self.ptype, m, x, self.alpha[s0], self.sigma[s0]).astype(F32)
        if inv_r0 is None:
            x_t = ratio * x - ah * x0
        else:
            d1 = inv_r0 * (x0 - self.x0_prev)
            x_t = ratio * x - ah * x0 - F32(0.5) * ah * d1
        self.x0_prev = x0
        return x_t.astype(F32)

