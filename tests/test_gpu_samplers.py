"""DPM-Solver++, trailing / linspace DDIM and guidance rescale on a real MI355X: the rescale-factor kernel against torch, the fused
update kernel (`sdt_sampler_cfg_step`) step by step against the float32 restatement (tests/sampler_reference.py) and the DDIM
oracle, an exact-answer run that needs no reference, and `generate()` on the tiny configuration against a restated loop over
oracle.nets.  Tolerances: kernel arithmetic is fp32 (1e-5); the networks compute in bf16 against an fp32 oracle (the gates of
test_gpu_sampling.py)."""
import numpy as np
import pytest
import torch

from tests import sampler_reference as ref
from tests.helpers import build_hip_states, make_case, rel_l2

pytestmark = pytest.mark.gpu

SL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
ZSNR = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="zero_snr_scaled_linear")


@pytest.fixture(scope="module")
def dev():
    from stable_diffusion_training_amd import _lib
    _lib.require_device()
    return torch.device("cuda:0")


def _random_pred(gen, B, C, h, w, cpad, pad_value=0.0):
    """bf16-representable (2B,h,w,cpad) UNet output; padding channels hold pad_value (the kernels must ignore them)."""
    pred = torch.full((2 * B, h, w, cpad), pad_value)
    pred[..., :C] = torch.randn(2 * B, h, w, C, generator=gen)
    return pred.to(torch.bfloat16).float()


def _halves(pred, B, C):
    return pred[:B, ..., :C].permute(0, 3, 1, 2), pred[B:, ..., :C].permute(0, 3, 1, 2)


def _check_next_input(d_next, d_lat, B, C):
    nxt = d_next.float().cpu()
    assert torch.equal(nxt[:B], nxt[B:]) and float(nxt[..., C:].abs().max()) == 0.0
    assert torch.equal(nxt[:B, ..., :C], d_lat.cpu().to(torch.bfloat16).float().permute(0, 2, 3, 1))


# ----------------------------------------------------------------------------- 1. rescale factors
@pytest.mark.parametrize("B,C,cpad", [(1, 4, 8), (4, 4, 16), (3, 9, 16)])
def test_rescale_factors_match_torch(dev, B, C, cpad):
    from stable_diffusion_training_amd import _lib
    h, w, g, phi = 5, 7, 7.5, 0.7
    gen = torch.Generator().manual_seed(B * 100 + cpad)
    pred = _random_pred(gen, B, C, h, w, cpad, pad_value=1e4)
    pred[:, ..., :C] *= torch.linspace(0.5, 3.0, 2 * B).view(-1, 1, 1, 1).to(torch.bfloat16).float()  # unequal stds per row
    if B > 1:  # sample 0: un == tx == constant -> std(cfg) == 0 -> factor 1
        pred[0, ..., :C] = 0.25
        pred[B, ..., :C] = 0.25
    pred = pred.to(torch.bfloat16).float()  # what the device holds
    un, tx = _halves(pred, B, C)
    cfg = un + g * (tx - un)
    want_out = ref.rescale_noise_cfg(cfg.double(), tx.double(), phi)  # diffusers' formula, float64
    want = ref.rescale_factors(un, tx, g, phi)
    d_pred = pred.to(dev, torch.bfloat16)
    f = torch.full((B,), -1.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("sdt_cfg_rescale_factors", d_pred.data_ptr(), f.data_ptr(), B, C, h, w, cpad, g, phi, stream)
    got = f.cpu().double()
    if B > 1:
        assert got[0] == 1.0
        want[0] = 1.0
    assert torch.allclose(got, want, rtol=1e-5, atol=0), (got, want)
    rows = slice(1, None) if B > 1 else slice(None)
    got_out = cfg.double()[rows] * got[rows].view(-1, 1, 1, 1)
    assert torch.allclose(got_out, want_out[rows], rtol=1e-5, atol=1e-5)
    f2 = torch.full((B,), -1.0, device=dev)
    _lib.call("sdt_cfg_rescale_factors", d_pred.data_ptr(), f2.data_ptr(), B, C, h, w, cpad, g, phi, stream)
    assert torch.equal(f.cpu(), f2.cpu())  # fixed reduction order: bitwise the same
    _lib.call("sdt_cfg_rescale_factors", d_pred.data_ptr(), f2.data_ptr(), B, C, h, w, cpad, g, 0.0, stream)
    assert torch.equal(f2.cpu(), torch.ones(B))


# ----------------------------------------------------------------------------- 2. DPM-Solver++ sequences
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("n", [6, 16])
@pytest.mark.parametrize("ptype", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_solver_sequence_matches_restatement(dev, order, ptype, n, phi):
    from stable_diffusion_training_amd.schedulers import DPMSolverMultistepScheduler
    B, C, h, w, cpad, g = 2, 4, 5, 7, 8, 4.0
    sched = SL if ptype == "epsilon" else ZSNR  # the zero-SNR rows (t = 999, lambda = -inf) for sample / v
    sch = DPMSolverMultistepScheduler(**sched, prediction_type=ptype, solver_order=order)
    ts = sch.set_timesteps(n)
    r = ref.DPMSolverPP(sch.alphas_cumprod, ts, ptype, order)
    gen = torch.Generator().manual_seed(order * 1000 + n * 10 + int(phi * 10))
    lat = torch.randn(B, C, h, w, generator=gen)
    d_lat = lat.to(dev)
    d_next = torch.full((2 * B, h, w, cpad), 7.0, dtype=torch.bfloat16, device=dev)
    for i, t in enumerate(ts):
        pred = _random_pred(gen, B, C, h, w, cpad)
        un, tx = _halves(pred, B, C)
        x = d_lat.cpu().clone()
        sch.cfg_step(pred.to(dev, torch.bfloat16), d_lat, d_next, t, g, phi)
        want = r.step(i, ref.guided(un, tx, g, phi).numpy(), x.numpy())
        got = d_lat.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5), (i, int(t), np.abs(got - want).max())
        _check_next_input(d_next, d_lat, B, C)
    assert sch.x0_history is not None and tuple(sch.x0_history.shape) == (B, C, h, w)
    assert np.allclose(sch.x0_history.cpu().numpy(), r.x0_prev, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------- 3. DDIM trailing / linspace through the new kernel
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("ptype", ["epsilon", "sample", "v_prediction"])
@pytest.mark.parametrize("spacing,n", [("trailing", 7), ("linspace", 6)])
def test_ddim_spacings_match_oracle(dev, spacing, n, ptype, phi):
    from oracle import schedulers as osched
    from stable_diffusion_training_amd.schedulers import DDIMScheduler
    B, C, h, w, cpad, g = 2, 4, 5, 7, 8, 7.5
    sname = "scaled_linear" if ptype == "epsilon" else "zero_snr_scaled_linear"
    sch = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule=sname, prediction_type=ptype, timestep_spacing=spacing)
    state = osched.create_state(sname)
    ts = sch.set_timesteps(n)
    assert ts[0] == 999 and (ptype == "epsilon") == (state["alphas_cumprod"][999] > 0)
    gen = torch.Generator().manual_seed(n * 7 + len(ptype) + int(phi * 10))
    d_lat = torch.randn(B, C, h, w, generator=gen).to(dev)
    d_next = torch.full((2 * B, h, w, cpad), 7.0, dtype=torch.bfloat16, device=dev)
    for t in ts:
        pred = _random_pred(gen, B, C, h, w, cpad)
        un, tx = _halves(pred, B, C)
        x = d_lat.cpu().numpy().copy()
        sch.cfg_step(pred.to(dev, torch.bfloat16), d_lat, d_next, t, g, phi)
        want = osched.ddim_step(state, ref.guided(un, tx, g, phi).numpy(), int(t), x, n, ptype)
        got = d_lat.cpu().numpy()
        assert np.all(np.isfinite(got))
        assert np.allclose(got, want, rtol=1e-5, atol=1e-5), (int(t), np.abs(got - want).max())
        _check_next_input(d_next, d_lat, B, C)


def test_ddim_leading_default_path_unchanged(dev):
    """Leading spacing without rescale still runs sdt_ddim_cfg_step: the same bits as calling it directly."""
    from stable_diffusion_training_amd import _lib
    from stable_diffusion_training_amd.schedulers import DDIMScheduler
    B, C, h, w, cpad = 2, 4, 5, 7, 8
    gen = torch.Generator().manual_seed(3)
    pred = _random_pred(gen, B, C, h, w, cpad).to(dev, torch.bfloat16)
    lat = torch.randn(B, C, h, w, generator=gen).to(dev)
    sch = DDIMScheduler(**SL, prediction_type="v_prediction")
    sch.set_timesteps(20)
    a, b = lat.clone(), lat.clone()
    na, nb = (torch.empty(2 * B, h, w, cpad, dtype=torch.bfloat16, device=dev) for _ in range(2))
    sch.cfg_step(pred, a, na, 500, 7.5)
    a_t, a_prev = sch.alpha_products(500)
    _lib.call("sdt_ddim_cfg_step", pred.data_ptr(), b.data_ptr(), nb.data_ptr(), B, C, h, w, cpad, 7.5, a_t, a_prev, 2,
              torch.cuda.current_stream().cuda_stream)
    assert torch.equal(a, b) and torch.equal(na, nb)


# ----------------------------------------------------------------------------- 4. exact answer
@pytest.mark.parametrize("sampler", ["dpmpp", "ddim"])
def test_exact_velocity_model_lands_on_data_point(dev, sampler):
    """Zero-SNR schedule, v-prediction, trailing timesteps, and a "model" that returns the exact velocity of one data point x*
    (v = alpha_t eps - sigma_t x* with eps = (x - alpha_t x*) / sigma_t, from the current latents).  With x = eps at t = 999,
    DDIM ends at x* and DPM-Solver++ at alpha_0 x* + sigma_0 eps (its last step goes to t = 0), up to the bf16 rounding of v."""
    from stable_diffusion_training_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    B, C, h, w, cpad, n = 2, 4, 6, 5, 8, 10
    kw = dict(ZSNR, prediction_type="v_prediction", timestep_spacing="trailing")
    sch = DPMSolverMultistepScheduler(**kw) if sampler == "dpmpp" else DDIMScheduler(**kw)
    gen = torch.Generator().manual_seed(11)
    x_star = torch.randn(B, C, h, w, generator=gen).to(dev)
    eps = torch.randn(B, C, h, w, generator=gen).to(dev)
    ac = torch.from_numpy(sch.alphas_cumprod).to(dev)
    lat = eps.clone()  # alpha_999 = 0: pure noise
    d_next = torch.empty(2 * B, h, w, cpad, dtype=torch.bfloat16, device=dev)
    pred = torch.zeros(2 * B, h, w, cpad, dtype=torch.bfloat16, device=dev)
    for t in sch.set_timesteps(n):
        a, s = ac[int(t)].sqrt(), (1 - ac[int(t)]).sqrt()
        v = a * (lat - a * x_star) / s - s * x_star
        pred[:B, ..., :C] = v.permute(0, 2, 3, 1).to(torch.bfloat16)
        pred[B:] = pred[:B]
        sch.cfg_step(pred, lat, d_next, t, 5.0, 0.0)
    if sampler == "dpmpp":
        a0, s0 = ac[0].sqrt(), (1 - ac[0]).sqrt()
        want = a0 * x_star + s0 * eps
    else:
        want = x_star
    err = float((lat - want).abs().max())
    assert err < 3e-2, err


# ----------------------------------------------------------------------------- 5. generate() against a restated loop
def _full_vae(case, seed=9):
    from oracle import nets as onets
    w = dict(case["weights"]["vae"])
    w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), seed))
    return w


def _oracle_generate(case, w_vae, ids, neg, lat0, timesteps, step, scale, phi):
    """oracle/sampling.generate with the update and the guidance rescale made pluggable (diffusers' rescale_noise_cfg order)."""
    from oracle import nets as onets
    with torch.no_grad():
        cfgs = case["cfgs"]
        pe = onets.clip_text_forward(case["weights"]["clip"], cfgs["clip"], torch.as_tensor(ids).long())
        ne = onets.clip_text_forward(case["weights"]["clip"], cfgs["clip"], torch.as_tensor(neg).long())
        ctx = torch.cat([ne, pe])
        lat = lat0.clone()
        for i, t in enumerate(timesteps):
            x2 = torch.cat([lat, lat])
            out = onets.unet_forward(case["weights"]["unet"], cfgs["unet"], x2, torch.full((x2.shape[0],), int(t), dtype=torch.int64), ctx)
            un, tx = out.chunk(2)
            m = un + scale * (tx - un)
            if phi > 0:
                m = ref.rescale_noise_cfg(m, tx, phi)
            lat = torch.from_numpy(step(i, int(t), m.numpy(), lat.numpy()))
        img = onets.vae_decode(w_vae, cfgs["vae"], (lat / 0.18215).permute(0, 2, 3, 1))
        return (img / 2 + 0.5).clamp(0, 1), lat


@pytest.mark.parametrize("sampler,spacing,ptype,sname,steps,phi", [
    ("dpmpp", "linspace", "v_prediction", "zero_snr_scaled_linear", 4, 0.7),
    ("ddim", "trailing", "v_prediction", "zero_snr_scaled_linear", 4, 0.7),
    ("dpmpp", "leading", "epsilon", "scaled_linear", 16, 0.0),
])
def test_generate_matches_restated_loop_tiny(dev, sampler, spacing, ptype, sname, steps, phi):
    from oracle import schedulers as osched
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    from stable_diffusion_training_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    case = make_case("tiny", B=2, image=64, sched=sname)
    tc, (us, ts, ue, te, vae, sc, objs) = build_hip_states(case, dev, prediction_type=ptype)
    w_vae = _full_vae(case)
    kw = dict(beta_start=0.00085, beta_end=0.012, beta_schedule=sname, prediction_type=ptype, timestep_spacing=spacing)
    sch = DPMSolverMultistepScheduler(**kw) if sampler == "dpmpp" else DDIMScheduler(**kw)
    pipe = StableDiffusionPipeline(us, ts, w_vae, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], scheduler=sch)
    timesteps = sch.set_timesteps(steps).copy()
    if sampler == "dpmpp":
        solver = ref.DPMSolverPP(sch.alphas_cumprod, timesteps, ptype)
        step = lambda i, t, m, x: solver.step(i, m, x)
    else:
        step = lambda i, t, m, x: osched.ddim_step(case["sched_state"], m, t, x, steps, ptype)
    ids = case["batch"]["input_ids"]
    vocab = case["cfgs"]["clip"]["vocab_size"]
    neg = torch.full_like(ids, vocab - 1)
    neg[:, 0] = vocab - 2
    lat0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    scale = 3.0
    want_img, want_lat = _oracle_generate(case, w_vae, ids, neg, lat0, timesteps, step, scale, phi)
    img, lat = pipe.generate(ids.to(dev), num_inference_steps=steps, height=64, width=64, guidance_scale=scale, latents=lat0.to(dev),
                             return_latents=True, guidance_rescale=phi)
    assert tuple(img.shape) == (2, 64, 64, 3) and bool(torch.isfinite(lat).all())
    assert rel_l2(lat, want_lat) < 3e-2
    assert float((img.cpu() - want_img).abs().mean()) < 1e-2
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe.generate(ids.to(dev), num_inference_steps=steps, height=64, width=64, guidance_rescale=1.5)


def test_sdxl_generate_dpm_solver_with_rescale_runs(dev):
    from oracle import nets as onets
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    from stable_diffusion_training_amd.schedulers import DPMSolverMultistepScheduler
    from tests.test_gpu_sdxl_conditioning import _case
    case = _case()
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, quantize=False)
    w_vae = dict(case["weights"]["vae"])
    w_vae.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    sch = DPMSolverMultistepScheduler(**ZSNR, prediction_type="v_prediction")
    pipe = StableDiffusionPipeline(us, ts, w_vae, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], scheduler=sch,
                                   scaling_factor=0.13025)
    lat0 = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))
    img, lat = pipe.generate(case["batch"]["input_ids"].to(dev), num_inference_steps=3, height=128, width=128, guidance_scale=5.0,
                             latents=lat0.to(dev), return_latents=True, guidance_rescale=0.7)
    assert tuple(img.shape) == (2, 128, 128, 3)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(lat).all())
    assert sch._step == 3 and float(lat.abs().max()) > 0
