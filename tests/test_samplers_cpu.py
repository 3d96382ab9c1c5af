"""Host side of the DPM-Solver++ / trailing-timestep / guidance-rescale sampling paths, no GPU: the timestep tables as known
answers (diffusers 0.21.4), the per-step coefficients that `sdt_sampler_cfg_step` receives against the float32 restatement in
tests/sampler_reference.py (zero-terminal-SNR rows included), the refusals, and the argument checks of the new entry points."""
import numpy as np
import pytest

from stable_diffusion_training_amd import _lib
from stable_diffusion_training_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from tests import sampler_reference as ref

SL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ZSNR = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="zero_snr_scaled_linear")
F = np.float32


# ----------------------------------------------------------------------------- timestep tables
def test_ddim_timestep_tables():
    lead = DDIMScheduler(**SL).set_timesteps(20)
    assert lead.tolist() == list(range(950, -1, -50))  # unchanged default
    assert lead.dtype == np.int32
    assert DDIMScheduler(**SL, timestep_spacing="trailing").set_timesteps(20).tolist() == list(range(999, 0, -50))
    assert DDIMScheduler(**SL, timestep_spacing="trailing").set_timesteps(7).tolist() == [999, 856, 713, 570, 428, 285, 142]
    lin = DDIMScheduler(**SL, timestep_spacing="linspace").set_timesteps(20).tolist()
    assert lin == [999, 946, 894, 841, 789, 736, 684, 631, 578, 526, 473, 421, 368, 315, 263, 210, 158, 105, 53, 0]


def test_ddim_previous_timestep_stays_t_minus_ratio():
    s = DDIMScheduler(**SL, timestep_spacing="trailing")
    s.set_timesteps(7)
    ac = s.alphas_cumprod
    assert s.alpha_products(999) == (float(ac[999]), float(ac[999 - 142]))
    assert s.alpha_products(142) == (float(ac[142]), float(ac[0]))
    s = DDIMScheduler(**SL, timestep_spacing="linspace")
    s.set_timesteps(20)
    assert s.alpha_products(946) == (float(ac[946]), float(ac[946 - 50]))
    assert s.alpha_products(0) == (float(ac[0]), 1.0)


def test_trailing_table_has_n_entries():
    # round(arange(1000, 0, -1000/61)) has a 62nd entry that is -1 after the shift; the table keeps the first 61
    for n in (1, 7, 48, 61, 103, 1000):
        ts = DDIMScheduler(**SL, timestep_spacing="trailing").set_timesteps(n)
        assert len(ts) == n and ts[0] == 999 and ts.min() >= 0 and np.all(np.diff(ts) < 0), n


def test_dpm_timestep_tables():
    lin = DPMSolverMultistepScheduler(**SL).set_timesteps(20).tolist()
    assert lin == [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50]
    lead = DPMSolverMultistepScheduler(**SL, timestep_spacing="leading").set_timesteps(20).tolist()
    assert lead == list(range(940, 0, -47))
    assert DPMSolverMultistepScheduler(**SL, timestep_spacing="leading", steps_offset=1).set_timesteps(20).tolist() == \
        list(range(941, 1, -47))
    assert DPMSolverMultistepScheduler(**SL, timestep_spacing="trailing").set_timesteps(20).tolist() == list(range(999, 0, -50))
    assert DPMSolverMultistepScheduler(**SL, timestep_spacing="trailing").set_timesteps(7).tolist() == \
        [999, 856, 713, 570, 428, 285, 142]


def test_dpm_repeated_timesteps_are_dropped():
    s = DPMSolverMultistepScheduler(**SL)
    ts = s.set_timesteps(1000)  # round(linspace(0, 999, 1001)) repeats one value
    assert len(ts) == 999 == s.num_inference_steps and len(np.unique(ts)) == 999 and np.all(np.diff(ts) < 0)
    raw = np.round(np.linspace(0, 999, 1001))[::-1][:-1].astype(np.int32)
    _, first = np.unique(raw, return_index=True)
    assert ts.tolist() == raw[np.sort(first)].tolist()


def test_sampling_tables():
    s = DPMSolverMultistepScheduler(**ZSNR, prediction_type="v_prediction")
    a, sg, lam = ref.tables(s.alphas_cumprod)
    assert s.alphas_cumprod[999] == 0.0
    assert np.array_equal(s.alpha_t, a) and np.array_equal(s.sigma_t, sg) and np.array_equal(s.lambda_t, lam)
    assert s.alpha_t.dtype == s.sigma_t.dtype == s.lambda_t.dtype == np.float32
    assert s.lambda_t[999] == -np.inf and np.all(np.isfinite(s.lambda_t[:999])) and np.all(np.diff(s.lambda_t) < 0)


# ----------------------------------------------------------------------------- coefficients
def _dpm_cases():
    for sched in (SL, ZSNR):
        for spacing in ("linspace", "leading", "trailing"):
            for n in (1, 2, 6, 14, 15, 16, 25):
                for order in (1, 2):
                    for lof in (True, False):
                        yield sched, spacing, n, order, lof


def test_dpm_coefficients_match_restatement():
    checked = 0
    for sched, spacing, n, order, lof in _dpm_cases():
        s = DPMSolverMultistepScheduler(**sched, prediction_type="v_prediction", solver_order=order, lower_order_final=lof,
                                        timestep_spacing=spacing)
        ts = s.set_timesteps(n)
        r = ref.DPMSolverPP(s.alphas_cumprod, ts, "v_prediction", order, lof)
        for i in range(len(ts)):
            c = s.step_coefficients(i)
            s0, t, ratio, ah, inv_r0 = r.terms(i)
            assert all(type(v) is np.float32 for v in c) and all(np.isfinite(c)), (spacing, n, i, c)
            assert c[0] == r.alpha[s0] and c[1] == r.sigma[s0]
            assert np.isclose(c[2], ratio, rtol=1e-6, atol=0) and np.isclose(c[3], -ah, rtol=1e-6, atol=0) and c[4] == 0
            if inv_r0 is None:
                assert c[5] == 0
            else:
                assert np.isclose(c[5], -F(0.5) * ah * inv_r0, rtol=1e-6, atol=1e-12), (spacing, n, i)
            checked += 1
    assert checked > 1000


def test_dpm_zero_snr_rows():
    s = DPMSolverMultistepScheduler(**ZSNR, prediction_type="v_prediction")
    ts = s.set_timesteps(20)
    assert ts[0] == 999
    a_s, sg_s, c_x, c_x0, c_eps, c_d1 = s.step_coefficients(0)  # h = +inf: e^-h = 0
    t = ts[1]
    assert a_s == 0 and sg_s == 1
    assert c_x == s.sigma_t[t] and c_x0 == s.alpha_t[t] and c_d1 == 0
    c = s.step_coefficients(1)  # r0 = +inf: 1 / r0 = 0, no 0 * inf
    assert all(np.isfinite(c)) and c[5] == 0
    c = s.step_coefficients(2)
    assert all(np.isfinite(c)) and c[5] != 0
    # the last step ends at t = 0, not at a clean sample
    c = s.step_coefficients(19)
    assert c[2] == s.sigma_t[0] / s.sigma_t[ts[19]] and c[2] > 0


def test_ddim_coefficients():
    for spacing in ("leading", "trailing", "linspace"):
        s = DDIMScheduler(**ZSNR, prediction_type="v_prediction", timestep_spacing=spacing)
        for t in s.set_timesteps(7):
            a_t, a_prev = (F(v) for v in s.alpha_products(t))
            c = s.step_coefficients(t)
            assert all(type(v) is np.float32 for v in c)
            assert c == (np.sqrt(a_t), np.sqrt(F(1) - a_t), 0, np.sqrt(a_prev), np.sqrt(F(1) - a_prev), 0)
    s = DDIMScheduler(**ZSNR, prediction_type="v_prediction", timestep_spacing="trailing")
    s.set_timesteps(20)
    assert s.step_coefficients(999)[:2] == (0, 1)


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    with pytest.raises(ValueError, match="epsilon"):
        DDIMScheduler(**ZSNR, timestep_spacing="trailing").set_timesteps(20)
    with pytest.raises(ValueError, match="epsilon"):
        DPMSolverMultistepScheduler(**ZSNR).set_timesteps(20)
    # leading spacing never visits t = 999 at 20 steps: an epsilon model of that schedule still samples there
    assert DPMSolverMultistepScheduler(**ZSNR, timestep_spacing="leading").set_timesteps(20)[0] == 940
    assert DDIMScheduler(**ZSNR).set_timesteps(20)[0] == 950
    for order in (0, 3):
        with pytest.raises(ValueError, match="solver_order"):
            DPMSolverMultistepScheduler(**SL, solver_order=order)
    with pytest.raises(ValueError, match="timestep_spacing"):
        DPMSolverMultistepScheduler(**SL, timestep_spacing="karras")
    with pytest.raises(ValueError, match="timestep_spacing"):
        DDIMScheduler(**SL, timestep_spacing="even")
    with pytest.raises(ValueError, match="prediction_type"):
        DPMSolverMultistepScheduler(**SL, prediction_type="flow")
    # guidance_rescale outside [0, 1] and out-of-order timesteps are refused before anything touches a tensor
    for sch in (DDIMScheduler(**SL, timestep_spacing="trailing"), DPMSolverMultistepScheduler(**SL)):
        sch.set_timesteps(20)
        for phi in (-0.1, 1.5):
            with pytest.raises(ValueError, match="guidance_rescale"):
                sch.cfg_step(None, None, None, 999, 7.5, phi)
    s = DPMSolverMultistepScheduler(**SL)
    with pytest.raises(ValueError, match="set_timesteps"):
        s.cfg_step(None, None, None, 999, 7.5)
    s.set_timesteps(20)
    with pytest.raises(ValueError, match="out of order"):
        s.cfg_step(None, None, None, 949, 7.5)
    s._step = 20
    with pytest.raises(ValueError, match="out of order"):
        s.cfg_step(None, None, None, 50, 7.5)
    s.set_timesteps(20)
    assert s._step == 0 and s.x0_history is None


# ----------------------------------------------------------------------------- C entry points without a GPU
def test_new_entry_points_validate_without_gpu(lib):
    assert lib.sdt_abi_version() == 5
    for name in ("sdt_cfg_rescale_factors", "sdt_sampler_cfg_step"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    P = 4096  # a non-null dummy address: every refusal below returns before any launch
    # sdt_sampler_cfg_step(pred, lat, next, hist, factors, B, C, H, W, cpad, g, alpha_s, sigma_s, ptype, c_x, c_x0, c_eps, c_d1, s)
    ok = dict(B=2, C=4, H=5, W=7, cpad=8, g=7.5, a=0.5, s=0.8, pt=2, cx=0.9, cx0=0.1, ceps=0.0, cd1=0.0)

    def step(pred=P, lat=P, nxt=P, hist=None, **kw):
        a = dict(ok, **kw)
        return lib.sdt_sampler_cfg_step(pred, lat, nxt, hist, None, a["B"], a["C"], a["H"], a["W"], a["cpad"], a["g"], a["a"], a["s"],
                                        a["pt"], a["cx"], a["cx0"], a["ceps"], a["cd1"], None)

    assert step(pred=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert step(pred=P + 8) == -1 and b"misaligned" in lib.sdt_last_error()
    assert step(cpad=12) == -1 and b"multiple of 8" in lib.sdt_last_error()
    assert step(C=9, cpad=8) == -1 and b"bad shape" in lib.sdt_last_error()
    assert step(pt=3) == -1 and b"prediction_type" in lib.sdt_last_error()
    assert step(a=1.5) == -1 and b"[0, 1]" in lib.sdt_last_error()
    assert step(a=float("nan")) == -1 and b"[0, 1]" in lib.sdt_last_error()
    assert step(pt=0, a=0.0, s=1.0) == -1 and b"epsilon prediction needs alpha_s" in lib.sdt_last_error()
    assert step(pt=1, a=1.0, s=0.0) == -1 and b"sample prediction needs sigma_s" in lib.sdt_last_error()
    assert step(cx0=float("inf")) == -1 and b"finite" in lib.sdt_last_error()
    assert step(cd1=float("nan")) == -1 and b"finite" in lib.sdt_last_error()
    assert step(g=float("inf")) == -1 and b"finite" in lib.sdt_last_error()
    assert step(cd1=0.5) == -1 and b"history" in lib.sdt_last_error()
    # sdt_cfg_rescale_factors(pred, factors, B, C, H, W, cpad, g, phi, stream)
    assert lib.sdt_cfg_rescale_factors(None, P, 2, 4, 5, 7, 8, 7.5, 0.7, None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_cfg_rescale_factors(P + 2, P, 2, 4, 5, 7, 8, 7.5, 0.7, None) == -1 and b"misaligned" in lib.sdt_last_error()
    assert lib.sdt_cfg_rescale_factors(P, P, 2, 4, 5, 7, 4, 7.5, 0.7, None) == -1 and b"bad shape" in lib.sdt_last_error()
    assert lib.sdt_cfg_rescale_factors(P, P, 2, 1, 1, 1, 8, 7.5, 0.7, None) == -1 and b"C*H*W >= 2" in lib.sdt_last_error()
    for phi in (-0.5, 1.01, float("nan")):
        assert lib.sdt_cfg_rescale_factors(P, P, 2, 4, 5, 7, 8, 7.5, phi, None) == -1 and b"[0, 1]" in lib.sdt_last_error()
    with pytest.raises(_lib.SdtError, match="sdt_sampler_cfg_step"):
        _lib.call("sdt_sampler_cfg_step", P, P, P, None, None, 2, 4, 5, 7, 8, 7.5, 0.0, 1.0, 0, 1.0, 1.0, 0.0, 0.0, None)
