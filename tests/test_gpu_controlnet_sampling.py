"""Sampling with a ControlNet on the MI355X: four steps of the tiny pipeline.  A zero-initialised ControlNet and a zero
conditioning_scale reproduce plain generate, a random ControlNet moves the result and its first-step prediction matches the CPU
reference on the doubled batch, and control_negative=False leaves the negative half to the plain UNet."""
import pytest
import torch

from tests import controlnet_reference as cr
from tests.helpers import build_hip_states, make_case, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TINY_CH = (16, 16, 32, 32)
STEPS = 4


@pytest.fixture(scope="module")
def world(dev):
    """One pipeline per ControlNet over the same UNet / text encoder / VAE stores, the inputs, and the plain result (computed once)."""
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev)
    w_vae = dict(case["weights"]["vae"])
    w_vae.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    ccfg = nets.controlnet_config(case["cfgs"]["unet"], TINY_CH)
    uw = case["weights"]["unet"]
    weights = dict(zero=nets.controlnet_from_unet(uw, ccfg, seed=6), random=cr.random_controlnet(uw, ccfg, seed=6))
    make = lambda cn: StableDiffusionPipeline(us, ts, w_vae, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], controlnet=cn)
    pipes = {k: make(dict(config=ccfg, params=w)) for k, w in weights.items()}
    pipes["plain"] = make(None)
    g = torch.Generator().manual_seed(4)
    inputs = dict(ids=case["batch"]["input_ids"].to(dev), lat0=torch.randn(2, 4, 8, 8, generator=g).to(dev),
                  hint=torch.rand(2, 3, 64, 64, generator=g).to(dev))
    aux = {}
    img, lat = pipes["plain"].generate(inputs["ids"], STEPS, 64, 64, guidance_scale=3.0, latents=inputs["lat0"], return_latents=True, aux=aux)
    return dict(case=case, ccfg=ccfg, weights=weights, pipes=pipes, plain=(img, lat, aux), **inputs)


def _run(world, which, **kw):
    aux = {}
    img, lat = world["pipes"][which].generate(world["ids"], STEPS, 64, 64, guidance_scale=3.0, latents=world["lat0"], return_latents=True,
                                              control_image=world["hint"], aux=aux, **kw)
    torch.cuda.synchronize()
    return img, lat, aux


def test_zero_initialised_controlnet_reproduces_plain_generate(world):
    img, lat, aux = _run(world, "zero")
    pimg, plat, paux = world["plain"]
    assert bool(torch.isfinite(plat).all()) and tuple(pimg.shape) == (2, 64, 64, 3)
    assert float(aux["control_mid"].abs().max()) == 0 and all(float(d.abs().max()) == 0 for d in aux["control_down"])
    assert torch.equal(aux["pred"], paux["pred"]) and torch.equal(lat, plat) and torch.equal(img, pimg)


def test_zero_conditioning_scale_reproduces_plain_generate(world):
    img, lat, aux = _run(world, "random", conditioning_scale=0.0)
    pimg, plat, paux = world["plain"]
    assert float(aux["control_mid"].abs().max()) > 0 and float(aux["control_scale"].abs().max()) == 0
    assert torch.equal(aux["pred"], paux["pred"]) and torch.equal(lat, plat) and torch.equal(img, pimg)


def test_random_controlnet_moves_the_result_and_matches_the_reference(world):
    img, lat, aux = _run(world, "random")
    pimg, plat, paux = world["plain"]
    assert bool(torch.isfinite(lat).all()) and not torch.equal(lat, plat) and not torch.equal(img, pimg)
    assert aux["control_scale"].tolist() == [1.0] * 4 and tuple(aux["unet_input"].shape) == (4, 8, 8, 8)
    assert torch.equal(aux["unet_input"], paux["unet_input"]) and torch.equal(aux["ctx"], paux["ctx"])
    # the reference on the doubled batch, fed the first step's own input, context and timesteps
    case = world["case"]
    x = aux["unet_input"][..., :4].float().cpu().permute(0, 3, 1, 2)
    t, ctx = aux["timesteps"].cpu().long(), aux["ctx"].float().cpu()
    hint = torch.cat([world["hint"], world["hint"]]).cpu().to(BF).float()
    down, mid = cr.controlnet_forward(world["weights"]["random"], world["ccfg"], x, t, ctx, hint)
    for a, b in zip(aux["control_down"] + [aux["control_mid"]], down + [mid]):
        assert rel_l2(a, b) < 2e-2
    ref = cr.unet_forward(case["weights"]["unet"], case["cfgs"]["unet"], x, t, ctx, down=down, mid=mid)
    plain_ref = cr.unet_forward(case["weights"]["unet"], case["cfgs"]["unet"], x, t, ctx)
    assert rel_l2(ref, plain_ref) > 0.05
    assert rel_l2(aux["pred"][..., :4].permute(0, 3, 1, 2), ref) < 2e-2


def test_control_on_the_prompt_half_only(world):
    img, lat, aux = _run(world, "random", control_negative=False, conditioning_scale=0.75)
    _, _, full = _run(world, "random", conditioning_scale=0.75)
    paux = world["plain"][2]
    assert aux["control_scale"].tolist() == [0.0, 0.0, 0.75, 0.75]
    assert torch.equal(aux["pred"][:2], paux["pred"][:2]), "the negative half saw the ControlNet"
    assert not torch.equal(aux["pred"][2:], paux["pred"][2:]) and torch.equal(aux["pred"][2:], full["pred"][2:])
    assert not torch.equal(full["pred"][:2], paux["pred"][:2])
    # the reference with the same scale vector
    case = world["case"]
    x = aux["unet_input"][..., :4].float().cpu().permute(0, 3, 1, 2)
    t, ctx = aux["timesteps"].cpu().long(), aux["ctx"].float().cpu()
    hint = torch.cat([world["hint"], world["hint"]]).cpu().to(BF).float()
    down, mid = cr.controlnet_forward(world["weights"]["random"], world["ccfg"], x, t, ctx, hint)
    ref = cr.unet_forward(case["weights"]["unet"], case["cfgs"]["unet"], x, t, ctx, down=down, mid=mid, scale=aux["control_scale"].cpu())
    assert rel_l2(aux["pred"][..., :4].permute(0, 3, 1, 2), ref) < 2e-2


def test_generate_refusals_on_the_device(world):
    with pytest.raises(ValueError, match="needs a pipeline built with controlnet="):
        world["pipes"]["plain"].generate(world["ids"], STEPS, 64, 64, control_image=world["hint"])
    with pytest.raises(ValueError, match="samples from a control_image"):
        world["pipes"]["zero"].generate(world["ids"], STEPS, 64, 64)
    with pytest.raises(ValueError, match="Unexpected control_image shape"):
        world["pipes"]["zero"].generate(world["ids"], STEPS, 64, 64, control_image=world["hint"][:, :, :32])
