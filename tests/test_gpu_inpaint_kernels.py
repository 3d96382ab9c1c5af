"""The three inpainting launches (include/sdt.h "INPAINTING") on the MI355X, bit for bit: sdt_inpaint_mask_pixels against the layout
conversion it replaces and the numpy reference, sdt_inpaint_noise_target against sdt_latent_noise_target and the posterior-sample
chain on the same operands, sdt_inpaint_pack_input against torch.cat on the host.  Guarded buffers, NaN-guarded inputs."""
import itertools

import numpy as np
import pytest
import torch

import tests.kernel_checks as kc
from tests import inpaint_reference as ir
from tests.kernel_checks import Guarded, assert_equal_bits

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _flat_in(data, dtype, dev, guard=float("nan")):
    return Guarded(1, data.numel(), dtype, dev, data=data.reshape(1, -1), guard=guard, pad=0, back_rows=0)


def _flat_out(n, dtype, dev):
    return Guarded(1, n, dtype, dev, pad=0, back_rows=0)


def _u16(t):
    """bf16 tensor -> numpy uint16 bit patterns."""
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _mask_values(shape, gen):
    """Values drawn from MASK_VALUES, every one of them present."""
    vals = torch.from_numpy(ir.MASK_VALUES)
    n = int(np.prod(shape))
    idx = torch.randint(0, len(vals), (n,), generator=gen)
    idx[: len(vals)] = torch.arange(len(vals))
    idx = idx[torch.randperm(n, generator=gen)]
    return vals[idx].reshape(shape)


# ================================================================================================ sdt_inpaint_mask_pixels
@pytest.mark.parametrize("H,W,f,cpad,shift", [(16, 24, 8, 8, 0), (5, 7, 1, 8, 0), (16, 24, 8, 3, 0), (16, 24, 8, 8, 4)],
                         ids=["vector", "odd_f1", "scalar_cpad3", "base_8_bytes_off"])
def test_mask_pixels_equals_the_layout_conversion_and_the_reference(dev, H, W, f, cpad, shift):
    """B = 2, C = 3.  shift: elements by which the stacked output's base is moved off its 16-byte alignment (4 bf16 = 8 bytes: the scalar
    store path at cpad 8)."""
    from stable_diffusion_training_amd import _lib
    B, C = 2, 3
    gen = torch.Generator().manual_seed(100 * H + W + cpad + shift)
    mask = _mask_values((B, H, W), gen)
    px = torch.randn(B, C, H, W, generator=gen)
    rp = torch.from_numpy(ir.repaint(mask.numpy()))
    ys, xs = rp[0].nonzero(as_tuple=True)
    px[0, 1, ys[0], xs[0]] = float("nan")  # a NaN and a -0 under the mask, a -0 outside it
    px[0, 2, ys[1], xs[1]] = -0.0
    yk, xk = (~rp[1]).nonzero(as_tuple=True)
    px[1, 0, yk[0], xk[0]] = -0.0
    assert (px < 0).any() and rp.any() and (~rp).any()
    PX, MK = _flat_in(px, F32, dev), _flat_in(mask, F32, dev)
    n = 2 * B * H * W * cpad
    ST, LM = _flat_out(n + 2 * shift, BF, dev), _flat_out(B * (H // f) * (W // f), F32, dev)
    _lib.call("sdt_inpaint_mask_pixels", PX.ptr, MK.ptr, ST.ptr + 2 * shift, LM.ptr, B, C, H, W, cpad, f, _stream())
    # what it replaces: the layout conversion of the image, and of the reference's masked image
    want_img = torch.empty(B, H, W, cpad, dtype=BF, device=dev)
    want_msk = torch.empty(B, H, W, cpad, dtype=BF, device=dev)
    masked = torch.from_numpy(ir.masked_image(px.numpy(), mask.numpy())).to(dev)
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", PX.ptr, want_img.data_ptr(), B, C, H, W, cpad, _stream())
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", masked.data_ptr(), want_msk.data_ptr(), B, C, H, W, cpad, _stream())
    torch.cuda.synchronize()
    for g in (PX, MK, ST, LM):
        g.check("mask_pixels")
    flat = ST.t.reshape(-1)
    sent = kc.SENTINEL[BF] - (1 << 16) if kc.SENTINEL[BF] >= 1 << 15 else kc.SENTINEL[BF]
    if shift:
        edge = torch.cat([flat[:shift], flat[shift + n:]]).view(torch.int16)
        assert (edge == sent).all(), "elements around the shifted output were written"
    got = flat[shift: shift + n].view(2 * B, H, W, cpad).cpu()
    assert_equal_bits(got[:B], want_img.cpu(), "image rows [image][row][column][channel]")
    assert_equal_bits(got[B:], want_msk.cpu(), "masked rows [image][row][column][channel]")
    assert (got[..., C:].view(torch.int16) == 0).all(), "padding channels not zero"
    under = got[B:][rp]  # (pixels under the mask, cpad)
    assert (under.view(torch.int16) == 0).all(), "a value other than +0 under the mask"
    assert torch.isnan(got[:B].float()).sum() == 1 and not torch.isnan(got[B:].float()).any()
    assert (got[B:].view(torch.int16) == -32768).sum() == 1, "the -0 outside the mask must survive (a select, not a multiply)"
    want_lm = torch.from_numpy(ir.latent_mask(mask.numpy(), f))
    assert_equal_bits(LM.t.view(B, H // f, W // f).cpu(), want_lm, "latent mask [image][row][column]")


# ================================================================================================ sdt_inpaint_noise_target
def _moments(P, L, ms, gen, nan_at):
    mom = torch.full((P, ms), float("nan"))
    mom[:, :L] = 2.0 * torch.randn(P, L, generator=gen)
    mom[:, L: 2 * L] = torch.rand(P, L, generator=gen) * 70.0 - 40.0  # [-40, 30): beyond -30 and 20
    mom[nan_at, L + 1] = float("nan")
    mom = mom.to(BF)
    lv = mom[:, L: 2 * L].float()
    assert (lv < -30).sum() > 3 and (lv > 20).sum() > 3 and torch.isnan(lv).sum() == 1
    return mom


@pytest.mark.parametrize("L,ms,cpad", [(4, 8, 16), (4, 16, 16), (4, 8, 24), (4, 9, 9), (3, 6, 8), (3, 6, 7), (16, 32, 40)])
def test_inpaint_noise_target_equals_the_plain_front_and_the_sample_chain(dev, L, ms, cpad):
    """B,H,W = 3,5,7; t = {0, 999, 500} of the zero-SNR schedule; log-variances beyond both clip bounds and one NaN in each moment
    tensor, NaN in the moment columns past 2L; mask values from the whole set.  For every prediction type x offset x perturbation x
    optional outputs: channels [0,L), target, latents and noisy carry sdt_latent_noise_target's bits from the same operands, channel L
    the thresholded mask, channels [L+1,2L+1) sdt_vae_posterior_sample of the masked moments through sdt_nchw_f32_to_nhwc_bf16, the rest
    zero, guards intact, and the row is the same with and without the optional outputs."""
    from oracle import schedulers as osched
    from stable_diffusion_training_amd import _lib
    B, H, W = 3, 5, 7
    P = B * H * W
    om, pm = 0.1, 0.07
    acp = torch.from_numpy(np.asarray(osched.create_state("zero_snr_scaled_linear")["alphas_cumprod"], np.float32))
    assert acp[999] == 0
    t = torch.tensor([0, 999, 500], dtype=torch.int32)
    gen = torch.Generator().manual_seed(1000 * L + 10 * ms + cpad)
    mom, mmom = _moments(P, L, ms, gen, 7), _moments(P, L, ms, gen, 40)
    eps, meps = torch.randn(P, L, generator=gen), torch.randn(P, L, generator=gen)
    noise = torch.randn(B, L, H, W, generator=gen)
    off, pn = torch.randn(B, L, 1, 1, generator=gen), torch.randn(B, L, H, W, generator=gen)
    lmask = _mask_values((B, H, W), gen)
    M, MM = Guarded(P, ms, BF, dev, data=mom, pad=0), Guarded(P, ms, BF, dev, data=mmom, pad=0)
    E, ME = Guarded(P, L, F32, dev, data=eps, pad=0), Guarded(P, L, F32, dev, data=meps, pad=0)
    N, OF, PN, LMK = _flat_in(noise, F32, dev), _flat_in(off, F32, dev), _flat_in(pn, F32, dev), _flat_in(lmask, F32, dev)
    T, A = _flat_in(t, torch.int32, dev, guard=0), _flat_in(acp, F32, dev)
    n_el = B * L * H * W

    # the masked-image latents, once: the posterior sample and the layout conversion's rounding
    mlat_w = torch.empty(B, L, H, W, dtype=F32, device=dev)
    mlat_b = torch.empty(B, H, W, L, dtype=BF, device=dev)
    _lib.call("sdt_vae_posterior_sample", MM.ptr, ME.ptr, mlat_w.data_ptr(), B, L, H, W, ms, kc.POST_SCALE, _stream())
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", mlat_w.data_ptr(), mlat_b.data_ptr(), B, L, H, W, L, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(mlat_w).sum() == 1
    for ptype, use_off, use_pn in itertools.product((0, 2), (False, True), (False, True)):
        what = f"ptype {ptype} offset {use_off} perturbation {use_pn}"
        ops = (OF.ptr if use_off else None, PN.ptr if use_pn else None, T.ptr, A.ptr)
        mags = (kc.POST_SCALE, om if use_off else 0.0, pm if use_pn else 0.0, ptype, _stream())
        nb_w = torch.empty(B, H, W, cpad, dtype=BF, device=dev)
        tg_w, lt_w, nz_w = (torch.empty(B, L, H, W, dtype=F32, device=dev) for _ in range(3))
        _lib.call("sdt_latent_noise_target", M.ptr, E.ptr, N.ptr, *ops, nb_w.data_ptr(), tg_w.data_ptr(), lt_w.data_ptr(), nz_w.data_ptr(),
                  B, L, H, W, ms, cpad, *mags)
        torch.cuda.synchronize()
        want = torch.from_numpy(ir.unet_input_bits(_u16(nb_w), lmask.numpy(), _u16(mlat_b), L, cpad).view(np.int16)).view(BF)
        plain = ptype == 0 and not use_off and not use_pn
        rows = []
        for full in (True, False):
            X = Guarded(P, cpad, BF, dev, pad=0)
            TG = None if (plain and not full) else _flat_out(n_el, F32, dev)  # the target may be NULL exactly there
            LT, NZ, ML = (_flat_out(n_el, F32, dev) for _ in range(3)) if full else (None, None, None)
            ptr = lambda g: None if g is None else g.ptr
            _lib.call("sdt_inpaint_noise_target", M.ptr, MM.ptr, E.ptr, ME.ptr, LMK.ptr, N.ptr, *ops, X.ptr, ptr(TG), ptr(LT), ptr(NZ), ptr(ML),
                      B, L, H, W, ms, cpad, *mags)
            torch.cuda.synchronize()
            X.check(f"{what}: input row")
            x = X.t.view(B, H, W, cpad).cpu()
            assert_equal_bits(x, want, f"{what} full {full}: UNet input [image][row][column][channel]")
            assert (x[..., 2 * L + 1:].view(torch.int16) == 0).all(), f"{what}: padding channels not zero"
            assert_equal_bits(x[..., :L].contiguous(), nb_w[..., :L].cpu().contiguous(), f"{what}: noisy channels vs sdt_latent_noise_target")
            if TG is not None:
                TG.check(f"{what}: target")
                assert_equal_bits(TG.t.view(B, L, H, W).cpu(), tg_w.cpu(), f"{what} full {full}: target NCHW")
            if full:
                for g, w_, name in ((LT, lt_w, "latents"), (NZ, nz_w, "noisy fp32"), (ML, mlat_w, "masked latents")):
                    g.check(f"{what}: {name}")
                    assert_equal_bits(g.t.view(B, L, H, W).cpu(), w_.cpu(), f"{what}: {name} NCHW")
            rows.append(x)
        assert_equal_bits(rows[1], rows[0], f"{what}: the row with and without the optional outputs")
    for g in (M, MM, E, ME, N, OF, PN, LMK, T, A):
        g.check("input")


# ================================================================================================ sdt_inpaint_pack_input
@pytest.mark.parametrize("double", [True, False], ids=["R=2B", "R=B"])
@pytest.mark.parametrize("L,cs,cm,cd", [(4, 8, 8, 16), (4, 8, 4, 9), (3, 8, 8, 8)])
def test_pack_input_equals_torch_cat(dev, L, cs, cm, cd, double):
    from stable_diffusion_training_amd import _lib
    B, h, w = 2, 5, 7
    R = 2 * B if double else B
    gen = torch.Generator().manual_seed(L * 1000 + cs * 100 + cm * 10 + cd + R)
    lat, mlat = torch.randn(R, h, w, cs, generator=gen).to(BF), torch.randn(B, h, w, cm, generator=gen).to(BF)
    lat[..., L:] = float("nan")  # the channels past L of either source must not travel
    mlat[..., L:] = float("nan")
    lat[0, 0, 0, 0], mlat[1, 2, 3, 1] = float("nan"), -0.0  # ... and a NaN and a -0 inside them travel as they are
    lmask = _mask_values((B, h, w), gen)
    LA, ML = Guarded(R * h * w, cs, BF, dev, data=lat, pad=0), Guarded(B * h * w, cm, BF, dev, data=mlat, pad=0)
    LMK, X = _flat_in(lmask, F32, dev), Guarded(R * h * w, cd, BF, dev, pad=0)
    _lib.call("sdt_inpaint_pack_input", LA.ptr, ML.ptr, LMK.ptr, X.ptr, R, B, L, h, w, cs, cm, cd, _stream())
    torch.cuda.synchronize()
    for g in (LA, ML, LMK, X):
        g.check("pack_input")
    rep = R // B
    mk = torch.from_numpy(ir.repaint(lmask.numpy())).to(BF)[..., None]
    want = torch.cat([lat[..., :L], mk.repeat(rep, 1, 1, 1), mlat[..., :L].repeat(rep, 1, 1, 1),
                      torch.zeros(R, h, w, cd - 2 * L - 1, dtype=BF)], dim=3)
    assert_equal_bits(X.t.view(R, h, w, cd).cpu(), want, "packed input [row][y][x][channel]")
    assert np.array_equal(_u16(want), ir.unet_input_bits(_u16(lat), lmask.numpy(), _u16(mlat), L, cd))
