"""The input rule of DESIGN.md 4 in numpy, one fp32 operation at a time (not a test module: test_input_cases_cpu.py pins it to the oracle
and to itself, test_gpu_input_exact.py compares csrc/preproc.hip with it bit for bit).  Every intermediate is an np.float32 -- nothing is
contracted, nothing kept wider, float64 nowhere: preproc.hip is built without contraction, its divisions are IEEE divisions, so it
performs these operations and no others.  `bilinear_taps` and `blend` are gaussian_cases', the arithmetic of `src_index` and of the
blend expression in the same order.  Written from the rule and the kernels' source text, never from a kernel's output.

An image is float32 planes (3,H,W) or bytes (H,W,3); a byte means its `table()` value.  Also the cases the CPU and the GPU tests share."""
import numpy as np
import torch

from gaussian_cases import F, bilinear_taps, blend            # tests/gaussian_cases.py

IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)             # the detector's transform
TANH_MEAN, TANH_STD = tuple(m * 2 - 1 for m in IMAGE_MEAN), tuple(s * 2 for s in IMAGE_STD)      # the embedder's input, on [-1, 1]
PAD = F(0.5)
STORAGE = {'bf16': torch.bfloat16, 'fp16': torch.float16}

# The largest differences between this model (fp32, before narrowing) and the oracle over ORACLE_TRANSFORMS / `oracle_boxes`, measured
# on the host by test_input_cases_cpu.py (printed there), times 2 -- for another torch build's interpolate summing in another order --
# and rounded up.  No kernel enters them.
#   transform: 7.99e-6 on 37 x 53, 9.33e-6 on 64 x 48, 1.264e-4 on 300 x 517 (there the oracle's 1 / scale_factor and in / out differ)
#   crops, mode 0: 1.19e-7 (2 units in the last place below 1); normalised: 7.15e-7
T_TRANSFORM_REF = {(37, 53): 1.6e-5, (64, 48): 1.9e-5, (300, 517): 2.6e-4}
T_CROP_REF = 2.4e-7
T_CROP_NORM_REF = 1.5e-6


def table():
    """the 256 float32 values of the 8-bit codes"""
    return (np.arange(256).astype(F) / F(255)).astype(F)


def planes(img):
    """either image form -> float32 planes (3,H,W)"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        assert img.ndim == 3 and img.shape[2] == 3
        return np.ascontiguousarray(table()[img].transpose(2, 0, 1))
    assert img.dtype == F and img.ndim == 3 and img.shape[0] == 3
    return img


def f3(values):
    """three Python floats, rounded to fp32 once -> (3,1,1)"""
    return np.array([F(v) for v in values], dtype=F).reshape(3, 1, 1)


def narrow(a, dtype):
    """fp32 -> the storage bits (int16) of bf16 | fp16, round to nearest even (torch's CPU cast; test_input_cases_cpu.py checks it
    against the bit-level rule)"""
    a = np.ascontiguousarray(a, dtype=F)
    return torch.from_numpy(a).to(dtype).view(torch.int16).numpy()


# ---- the detector's transform --------------------------------------------------------------------------------------------------------
def transform_f32(img, h, w, mean, std):
    """-> (3,h,w) f32: every tap normalised as (p - mean) / std, then the blend (the order of transform_pixel)"""
    p = planes(img)
    n = ((p - f3(mean)).astype(F) / f3(std)).astype(F)
    y0, y1, ly0, ly1 = bilinear_taps(h, p.shape[1])            # scale = float32(H0) / float32(h)
    x0, x1, lx0, lx1 = bilinear_taps(w, p.shape[2])
    return np.stack([blend(c[y0][:, x0], c[y0][:, x1], c[y1][:, x0], c[y1][:, x1], ly0, ly1, lx0, lx1) for c in n])


def transform(img, h, w, Hp, Wp, mean, std, dtype):
    """-> (Hp,Wp,8) storage bits: channels 3..7 and everything outside h x w are +0"""
    out = np.zeros((Hp, Wp, 8), dtype=np.int16)
    out[:h, :w, :3] = narrow(transform_f32(img, h, w, mean, std), dtype).transpose(1, 2, 0)
    return out


# ---- the RoI crops ---------------------------------------------------------------------------------------------------------------------
def box_geometry(boxes, H0, W0):
    """(P,4) f32 xyxy -> int64 arrays x1, y1, cw, ch: truncated toward zero, clamped to the image, negative extents 0"""
    b = np.trunc(np.asarray(boxes, dtype=F).reshape(-1, 4)).astype(np.int64)
    x1, x2 = np.clip(b[:, 0], 0, W0), np.clip(b[:, 2], 0, W0)
    y1, y2 = np.clip(b[:, 1], 0, H0), np.clip(b[:, 3], 0, H0)
    return x1, y1, np.maximum(x2 - x1, 0), np.maximum(y2 - y1, 0)


def crop_f32(img, boxes, S):
    """-> (P,3,S,S) f32 in [0,1]: the crop, padded with 0.5 to a square at the top left, resized to S x S"""
    p = planes(img)
    x1, y1, cw, ch = box_geometry(boxes, p.shape[1], p.shape[2])
    out = np.full((len(x1), 3, S, S), PAD, dtype=F)
    for k in range(len(x1)):
        larger = int(max(cw[k], ch[k]))
        if larger == 0:
            continue                                            # every pixel is exactly 0.5
        sq = np.full((3, larger, larger), PAD, dtype=F)         # a tap with yy >= ch or xx >= cw is 0.5
        sq[:, :ch[k], :cw[k]] = p[:, y1[k]:y1[k] + ch[k], x1[k]:x1[k] + cw[k]]
        i0, i1, l0, l1 = bilinear_taps(S, larger)               # scale = float32(larger) / float32(S), rows and columns alike
        for c in range(3):
            out[k, c] = blend(sq[c][i0][:, i0], sq[c][i0][:, i1], sq[c][i1][:, i0], sq[c][i1][:, i1], l0, l1, l0, l1)
        # a pixel whose first taps lie in the padding is EXACTLY 0.5 (the weights sum to 1 only up to an ulp)
        out[k][:, (i0[:, None] >= ch[k]) | (i0[None, :] >= cw[k])] = PAD
    return out


def normalize_tanh_f32(v, mean, std):
    """(..,3,S,S) in [0,1] -> ((v * 2 - 1) - mean) / std, each operation rounded on its own"""
    t = ((v * F(2)).astype(F) - F(1)).astype(F)
    return ((t - f3(mean)).astype(F) / f3(std)).astype(F)


def nhwc(v, channels, dtype=torch.bfloat16):
    """(P,3,S,S) f32 -> (P,S,S,channels) storage bits, zero fill"""
    out = np.zeros((v.shape[0], v.shape[2], v.shape[3], channels), dtype=np.int16)
    out[..., :3] = narrow(v, dtype).transpose(0, 2, 3, 1)
    return out


def crop(img, boxes, S, mode, mean=None, std=None):
    """mode 0: (P,3,S,S) f32; mode 1 | 2: the normalised values as bf16 bits, (P,S,S,8) | (P,S,S,4)"""
    v = crop_f32(img, boxes, S)
    return v if mode == 0 else nhwc(normalize_tanh_f32(v, mean, std), 8 if mode == 1 else 4)


def extents(boxes, H0, W0, S, count=None, per_image=0):
    """-> (P,2) int32 (rows, cols): how many output rows have yy0 < ch and how many columns xx0 < cw, by looking at all S positions.
    count (with per_image > 0: one per image, per_image slots each): slots beyond it are (S, S)."""
    x1, y1, cw, ch = box_geometry(boxes, H0, W0)
    out = np.zeros((len(x1), 2), dtype=np.int32)
    larger = np.maximum(cw, ch)
    for m in np.unique(larger[larger > 0]):
        i0 = bilinear_taps(S, int(m))[0]
        sel = larger == m
        out[sel, 0] = (i0[None, :] < ch[sel][:, None]).sum(axis=1)
        out[sel, 1] = (i0[None, :] < cw[sel][:, None]).sum(axis=1)
    if count is not None:
        slot = np.arange(len(x1))
        live = slot % per_image < np.asarray(count)[slot // per_image] if per_image > 0 else slot < int(np.asarray(count).reshape(-1)[0])
        out[~live] = S
    return out


def pad_extents(images, pad=0.5):
    """(B,3,S,S) f32 -> (B,2) int32: rows / columns beyond which every pixel equals `pad` in all three channels"""
    content = (np.asarray(images, dtype=F) != F(pad)).any(axis=1)              # (B,S,S)
    out = np.zeros((content.shape[0], 2), dtype=np.int32)
    for b, c in enumerate(content):
        rows, cols = np.flatnonzero(c.any(axis=1)), np.flatnonzero(c.any(axis=0))
        out[b] = (rows[-1] + 1 if len(rows) else 0, cols[-1] + 1 if len(cols) else 0)
    return out


def pack(images, to_tanh, mean, std):
    """(B,3,S,S) f32 -> (B,S,S,8) bf16 bits of (v - mean) / std, v = images * 2 - 1 with to_tanh"""
    v = np.asarray(images, dtype=F)
    if to_tanh:
        return nhwc(normalize_tanh_f32(v, mean, std), 8)
    return nhwc(((v - f3(mean)).astype(F) / f3(std)).astype(F), 8)


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------
def byte_image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def float_image(seed, h, w):
    """fp32 values in [0, 1) with full mantissas (a byte image's 256 values exercise few roundings)"""
    return np.random.RandomState(seed).rand(3, h, w).astype(F)


def source(form, seed, h, w):
    return byte_image(seed, h, w) if form == 'u8' else float_image(seed, h, w)


# the detector's transform: (form, (H0, W0) -> (h, w)), all in one padded batch of TRANSFORM_HP x TRANSFORM_WP (wider than one 128-column
# workgroup: a row's second workgroup is partial)
TRANSFORM_HP, TRANSFORM_WP = 96, 160
TRANSFORMS = [('u8', (37, 53), (24, 35)),        # a downscale, byte rows of odd length
              ('f32', (64, 48), (80, 60)),       # an upscale
              ('u8', (40, 64), (40, 64)),        # identity: weights exactly 1 and 0
              ('f32', (32, 32), (64, 64)),       # every source index on .25 / .75
              ('u8', (32, 32), (16, 16)),        # ... on .5
              ('f32', (1, 1), (5, 7)),           # i1 clamps onto i0
              ('u8', (2, 3), (9, 160))]          # ... and the full batch width
TINY_COUNT, TINY_SRC, TINY_DST = 33, (8, 8), (16, 16)          # one call past the 32 images of a launch


def transform_sources():
    return [source(form, 100 + i, *hw) for i, (form, hw, _) in enumerate(TRANSFORMS)]


def tiny_sources():
    return [source('u8' if i % 3 else 'f32', 200 + i, *TINY_SRC) for i in range(TINY_COUNT)]


# what oracle.gln.transform_one can be compared on: it resizes to its own size (oracle.gln.resized_size)
ORACLE_TRANSFORMS = [('u8', (37, 53)), ('f32', (64, 48)), ('f32', (300, 517))]

CROP_IMAGES = [(37, 53), (40, 64)]
CROP_SIZES = [7, 8, 260]        # the one-pixel kernel | two pixels per thread | two workgroups per row, an odd tail in the last thread
CROP_COUNTS = [9, 17]           # (the two-pixel kernel's grid z is rounded up to a multiple of 8)


def crop_boxes(h, w, S, n):
    """the first n of: tests/test_gpu_u8_kernels.py boxes_for(h, w), then the boxes that kernel was never shown"""
    b = [[0.0, 0.0, w, h],                            # the whole image
         [w - 1.0, h - 1.0, w, h],                    # 1 x 1 at the bottom-right pixel
         [w - 9.0, h - 7.0, w + 11.0, h + 5.0],       # hanging over the right and the bottom edge
         [-4.5, -2.25, 17.75, 20.5],                  # negative and fractional coordinates
         [3.3, 2.9, 30.6, 33.2],
         [12.0, 9.0, 12.0, 30.0],                     # zero area
         [5.0, 2.0, 8.0, 32.0],                       # tall, 3 x 30
         [4.0, 6.0, 34.0, 9.0],                       # wide, 30 x 3
         [1.0, 1.0, 20.0, 20.0],
         [30.0, 5.0, 10.0, 25.0],                     # reversed: x2 < x1
         [w + 3.0, h + 2.0, w + 20.0, h + 30.0],      # wholly outside the image
         [2.0, 1.0, 2.0 + min(S, w - 2), 4.0],        # larger == S (where the image holds it)
         [0.0, 3.0, min(2 * S, w), 9.0],              # larger == 2 S
         [6.0, 2.0, 6.0 + max(S // 2, 1), 3.0],       # larger == S / 2
         [20.0, 0.0, 31.0, h],                        # tall in a wide image: `larger` is the height
         [1.2, 1.2, 1.9, 1.9],                        # truncates to nothing
         [-0.9, -0.9, 0.9 + w, 0.9 + h]]              # truncates to the whole image
    assert n <= len(b)
    return np.array(b[:n], dtype=F)


def oracle_boxes(h, w, S=256):
    """the shared boxes the reference can crop: no negative corner (a Python slice would count from the end) and a positive area"""
    b = crop_boxes(h, w, S, 17)
    x1, y1, cw, ch = box_geometry(b, h, w)
    return b[(b[:, :2] >= 0).all(axis=1) & (cw > 0) & (ch > 0)]


# crop_extents: every integer box with corners in [-2, W0 + 2] x [-2, H0 + 2]
EXTENT_IMAGE = (9, 12)          # (H0, W0)
EXTENT_SIZES = [8, 256]


def extent_boxes():
    h, w = EXTENT_IMAGE
    xs, ys = np.arange(-2, w + 3), np.arange(-2, h + 3)
    g = np.stack(np.meshgrid(xs, ys, xs, ys, indexing='ij'), axis=-1).reshape(-1, 4)      # x1, y1, x2, y2
    return g.astype(F)
