"""The colour-jitter rule of include/simplerecon_hip.h ("frame preparation", part "colour jitter") in torch's CPU
operations: torchvision's published tensor path (ColorJitter.forward, functional_tensor's _blend, rgb_to_grayscale,
_rgb2hsv, _hsv2rgb) restated operation by operation, with to_tensor in front and the loader's flip and ImageNet
normalisation behind it.  torchvision is not installed where this was written: parity against the package itself is
unpinned.  Dtype-generic: run in float32 it rounds as torch rounds (what the loader computes), in float64 it is the
reference the tolerances are measured against.  scripts/bench_jitter.py runs the same functions on the device."""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def to_tensor(u8_bhwc, dtype=torch.float32):
    """uint8 [B,H,W,3] (numpy or torch) -> [B,3,H,W] of `dtype`: float(v) / 255."""
    return torch.as_tensor(u8_bhwc).permute(0, 3, 1, 2).contiguous().to(dtype).div(255)


def gray(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)


def blend(a, b, f):
    f = float(f)
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def brightness(img, f):
    return blend(img, torch.zeros_like(img), f)


def contrast(img, f):
    return blend(img, torch.mean(gray(img), dim=(-3, -2, -1), keepdim=True), f)


def saturation(img, f):
    return blend(img, gray(img), f)


def rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - (s * (1.0 - f)))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def hue(img, f):
    h, s, v = rgb2hsv(img).unbind(dim=-3)
    h = (h + float(f)) % 1.0
    return hsv2rgb(torch.stack((h, s, v), dim=-3))


OPERATORS = (brightness, contrast, saturation, hue)


def jitter_frame(img_3hw, order, factors, on):
    """ColorJitter.forward on one image [3,H,W] in [0, 1]: the operators that are `on`, in `order`."""
    for op in order:
        if on[int(op)]:
            img_3hw = OPERATORS[int(op)](img_3hw, float(factors[int(op)]))
    return img_3hw


def prepare(u8_bhwc, order, factors, on, flip=False, normalize=True, dtype=torch.float32):
    """The loader's colour path on B resized 8-bit images: to_tensor, the frame's jitter (order [B,4], factors [B,4]
    indexed by operator, `on` four booleans), the flip, the normalisation.  [B,3,H,W] of `dtype`."""
    img = to_tensor(u8_bhwc, dtype)
    img = torch.stack([jitter_frame(img[i], order[i], factors[i], on) for i in range(img.shape[0])])
    if flip:
        img = torch.flip(img, (-1,))
    if normalize:
        mean = torch.as_tensor(MEAN, dtype=dtype, device=img.device).view(-1, 1, 1)
        std = torch.as_tensor(STD, dtype=dtype, device=img.device).view(-1, 1, 1)
        img = img.sub(mean).div(std)
    return img
