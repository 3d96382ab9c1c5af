"""Sampling from an inpainting UNet on the MI355X: generate(image=, mask=) with DDIM and DPM-Solver++ against a loop written here from
nets.unet_forward, scheduler.cfg_step and torch.cat - bit for bit -, all-zero and all-one masks, and the refusals."""
import pytest
import torch

from tests import inpaint_reference as ir
from tests.helpers import build_hip_states, make_case
from tests.test_gpu_inpaint import _inpaint_case, _rect_masks

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SL = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon")


def _full_vae(case, seed=9):
    from oracle import nets as onets
    w = dict(case["weights"]["vae"])
    w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), seed))
    return w


def _scheduler(name):
    from stable_diffusion_training_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    return DDIMScheduler(**SL) if name == "ddim" else DPMSolverMultistepScheduler(**SL)


def _pipe(case, dev, sampler):
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev)
    pipe = StableDiffusionPipeline(us, ts, _full_vae(case), case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"],
                                   scheduler=_scheduler(sampler))
    return pipe, us, ts, vae


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp"])
def test_generate_equals_a_loop_of_unet_cfg_step_and_cat(dev, sampler):
    from stable_diffusion_training_amd import _lib, nets, ops
    case = _inpaint_case()
    pipe, us, ts, vae = _pipe(case, dev, sampler)
    stream = torch.cuda.current_stream().cuda_stream
    B, L, h, w, scale, steps = 2, 4, 8, 8, 3.0, 3
    g = torch.Generator().manual_seed(4)
    lat0, meps = torch.randn(B, L, h, w, generator=g).to(dev), torch.randn(B, h, w, L, generator=g).to(dev)
    image, mask = case["batch"]["pixel_values"].to(dev), case["batch"]["inpaint_mask"].to(dev)
    ids = case["batch"]["input_ids"].to(dev)
    img, lat = pipe.generate(ids, num_inference_steps=steps, height=64, width=64, guidance_scale=scale, latents=lat0, return_latents=True,
                             image=image, mask=mask, masked_eps=meps)
    torch.cuda.synchronize()
    assert tuple(img.shape) == (B, 64, 64, 3) and tuple(lat.shape) == (B, L, h, w) and bool(torch.isfinite(img).all())

    # the same, by hand
    vocab = case["cfgs"]["clip"]["vocab_size"]
    neg = torch.full_like(ids, vocab - 1)
    neg[:, 0] = vocab - 2
    us.store.prepare()
    ts.store.prepare()
    ctx = nets.clip_text_forward(ts.store, ts.config, torch.cat([neg, ids]).to(torch.int32)).detach()
    masked = torch.where((mask >= 0.5)[:, None], torch.zeros_like(image), image).contiguous()
    pix = torch.empty(B, 64, 64, 8, dtype=BF, device=dev)
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", masked.data_ptr(), pix.data_ptr(), B, 3, 64, 64, 8, stream)
    ops.gn_arena_begin(dev)
    moments = nets.vae_encode_moments(vae.params, vae.call, pix)
    ops.gn_arena_end(dev)
    mlat = torch.empty(B, L, h, w, dtype=F32, device=dev)
    _lib.call("sdt_vae_posterior_sample", moments.data_ptr(), meps.data_ptr(), mlat.data_ptr(), B, L, h, w, moments.shape[3], 0.18215, stream)
    mlat2 = mlat.to(BF).permute(0, 2, 3, 1).repeat(2, 1, 1, 1)
    mk2 = torch.from_numpy(ir.latent_mask(mask.cpu().numpy(), 8)).to(dev).to(BF)[..., None].repeat(2, 1, 1, 1)
    sch = _scheduler(sampler)
    cur = (lat0 * sch.init_noise_sigma).contiguous().clone()
    x_lat = torch.empty(2 * B, h, w, 8, dtype=BF, device=dev)
    for half in (x_lat[:B], x_lat[B:]):
        _lib.call("sdt_nchw_f32_to_nhwc_bf16", cur.data_ptr(), half.data_ptr(), B, L, h, w, 8, stream)
    t_dev = torch.empty(2 * B, dtype=torch.int32, device=dev)
    with torch.no_grad():
        for t in sch.set_timesteps(steps):
            t_dev.fill_(int(t))
            x_in = torch.cat([x_lat[..., :L], mk2, mlat2, torch.zeros(2 * B, h, w, 16 - 2 * L - 1, dtype=BF, device=dev)], dim=3).contiguous()
            ops.gn_arena_begin(dev)
            pred = nets.unet_forward(us.store, us.config, x_in, t_dev, ctx)
            ops.gn_arena_end(dev)
            sch.cfg_step(pred, cur, x_lat, t, scale)
    torch.cuda.synchronize()
    assert torch.equal(lat, cur), f"generate differs from the hand-written loop ({(lat - cur).abs().max().item():.3e} max abs)"
    assert not torch.equal(lat, lat0)


def test_all_zero_and_all_one_masks_run_finite_and_draw_from_the_generator(dev):
    case = _inpaint_case()
    pipe, us, ts, vae = _pipe(case, dev, "ddim")
    image, ids = case["batch"]["pixel_values"].to(dev), case["batch"]["input_ids"].to(dev)
    outs = []
    for value in (0.0, 1.0, 1.0):
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        img, lat = pipe.generate(ids, num_inference_steps=3, height=64, width=64, guidance_scale=3.0, generator=gen, return_latents=True,
                                 image=image, mask=torch.full((2, 64, 64), value, device=dev))
        assert tuple(lat.shape) == (2, 4, 8, 8) and bool(torch.isfinite(lat).all()) and bool(torch.isfinite(img).all())
        outs.append(lat.clone())
    assert torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[1])


def test_refusals(dev):
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = _inpaint_case()
    pipe, us, ts, vae = _pipe(case, dev, "ddim")
    image, ids = case["batch"]["pixel_values"].to(dev), case["batch"]["input_ids"].to(dev)
    mask = _rect_masks(2, 64, 64, 1).to(dev)
    gen = lambda **kw: pipe.generate(ids, num_inference_steps=2, height=64, width=64, **kw)
    for kw in (dict(), dict(image=image), dict(mask=mask)):
        with pytest.raises(ValueError, match="samples from an image and a mask"):
            gen(**kw)
    for kw in (dict(image=image[:1], mask=mask), dict(image=image[:, :, :32], mask=mask), dict(image=image[:, :2], mask=mask)):
        with pytest.raises(ValueError, match="Unexpected image shape"):
            gen(**kw)
    for kw in (dict(image=image, mask=mask[:, :8, :8]), dict(image=image, mask=mask[:, None]), dict(image=image, mask=mask[:1])):
        with pytest.raises(ValueError, match="Unexpected mask shape"):
            gen(**kw)
    with pytest.raises(ValueError, match="Unexpected masked_eps shape"):
        gen(image=image, mask=mask, masked_eps=torch.zeros(2, 4, 8, 8, device=dev))
    with pytest.raises(ValueError, match="Unexpected latents shape"):
        gen(image=image, mask=mask, latents=torch.zeros(2, 9, 8, 8, device=dev))
    # a plain UNet refuses the new arguments
    plain = make_case("tiny", B=2, image=64)
    tc, (us4, ts4, _, _, _, _, _) = build_hip_states(plain, dev)
    pipe4 = StableDiffusionPipeline(us4, ts4, _full_vae(plain), plain["cfgs"]["unet"], plain["cfgs"]["clip"], plain["cfgs"]["vae"])
    for kw in (dict(image=image, mask=mask), dict(mask=mask), dict(image=image)):
        with pytest.raises(ValueError, match="need an inpainting UNet"):
            pipe4.generate(ids, num_inference_steps=2, height=64, width=64, **kw)
