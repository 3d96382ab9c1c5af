"""numpy restatement of the data layout of include/sdt.h "INPAINTING": the mask threshold, the nearest-neighbour latent mask, the
masked image and the UNet input row [noisy latents | mask | masked-image latents | zero padding].  Nothing here rounds: the bf16
values that enter a row are produced by the launches they are compared with, and travel as uint16 bit patterns."""
import numpy as np

MASK_VALUES = np.array([0.0, 0.25, np.nextafter(np.float32(0.5), np.float32(0.0)), 0.5, 0.75, 1.0, -1.0, 2.0, np.nan], np.float32)
BF16_ONE = 0x3F80


def repaint(mask):
    """1 repaints, 0 keeps: m >= 0.5; a NaN compares false and keeps."""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, np.float32) >= np.float32(0.5)


def latent_mask(mask, f):
    """mask (B,H,W) -> float32 (B,H/f,W/f): the top-left pixel of every f x f block, thresholded (F.interpolate mode="nearest")."""
    B, H, W = mask.shape
    assert H % f == 0 and W % f == 0
    return repaint(mask[:, ::f, ::f]).astype(np.float32)


def masked_image(pixels, mask):
    """pixels float32 (B,C,H,W), mask (B,H,W) -> repaint ? +0.0 : x, a select: no -0 and no NaN survives under the mask."""
    return np.where(repaint(mask)[:, None, :, :], np.float32(0.0), np.asarray(pixels, np.float32)).astype(np.float32)


def nhwc_bits(x_nchw_bits, cpad):
    """uint16 (B,C,H,W) bit patterns -> (B,H,W,cpad), zero padded."""
    B, C, H, W = x_nchw_bits.shape
    out = np.zeros((B, H, W, cpad), np.uint16)
    out[..., :C] = x_nchw_bits.transpose(0, 2, 3, 1)
    return out


def unet_input_bits(noisy_bits, lmask, masked_bits, L, cpad):
    """The input rows as uint16 bit patterns (R,h,w,cpad).  noisy_bits (R,h,w,>=L) and masked_bits (B,h,w,>=L) are bf16 patterns of
    which the first L channels count, lmask (B,h,w) holds any float values (thresholded here).  Row r takes the mask and the masked
    latents of sample r % B (R a multiple of B: the doubled classifier-free-guidance batch)."""
    R, B = noisy_bits.shape[0], masked_bits.shape[0]
    assert R % B == 0 and cpad >= 2 * L + 1
    out = np.zeros(noisy_bits.shape[:3] + (cpad,), np.uint16)
    src = np.arange(R) % B
    out[..., :L] = noisy_bits[..., :L]
    out[..., L] = np.where(repaint(lmask)[src], BF16_ONE, 0).astype(np.uint16)
    out[..., L + 1: 2 * L + 1] = masked_bits[src][..., :L]
    return out
