"""The stroke rule of DESIGN.md 4b in plain numpy and Python integers, and the cases the stroke kernel is tested on.  (Not a test
module: test_strokes_cpu.py pins the model on the host, test_gpu_strokes.py compares csrc/strokes.hip with it byte for byte.)

The model paints FORWARD: stroke after stroke in list order, each over what is there -- the kernel searches backward from the last
stroke and stops at the first hit, so the two share the rule and nothing of its evaluation.  The model decides the third case of the
rule on Python integers (numpy object arrays), so no product can wrap: it needs no bound on |cross|.  It evaluates a stroke on the
pixels of its bounding box grown by the radius alone (a 32768-pixel canvas would otherwise cost 32768 tests per stroke);
test_strokes_cpu.py holds that window to a pixel-by-pixel evaluation of whole canvases.
"""
import numpy as np

TILE_W, TILE_H, CHUNK = 64, 16, 256
COLS = 6
MAX_SIDE = 32768
MAX_RADIUS = 64


def rgb_bytes(colour):
    return np.array([colour & 255, (colour >> 8) & 255, (colour >> 16) & 255], dtype=np.uint8)


def half(v):
    """a float32 coordinate in canvas pixels -> half pixels: floor(2 * clamp(v)), both exact in fp32"""
    v = np.clip(np.float32(v), np.float32(-32768), np.float32(32767))
    return int(np.floor(np.float32(2) * v))


def integers(ends, radius):
    """-> (ax, ay, bx, by, R) in half pixels, Python integers, or None where the stroke is skipped"""
    e = np.asarray(ends, dtype=np.float32)
    r = int(radius)
    if r <= 0 or not np.isfinite(e).all():
        return None
    return tuple(half(v) for v in e) + (min(r, MAX_RADIUS),)


def covers(stroke, x, y):
    """the rule for one pixel, Python integers throughout"""
    ax, ay, bx, by, r = stroke
    px, py = 2 * x + 1, 2 * y + 1
    dx, dy, vx, vy = bx - ax, by - ay, px - ax, py - ay
    l2, s = dx * dx + dy * dy, vx * dx + vy * dy
    if s <= 0:
        return vx * vx + vy * vy <= r * r
    if s >= l2:
        return (px - bx) ** 2 + (py - by) ** 2 <= r * r
    return (vx * dy - vy * dx) ** 2 <= r * r * l2


def covered(hw, ends, radius):
    """-> (y0, x0, mask) -- the pixels of the window canvas[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]] the stroke covers -- or None
    where it covers none"""
    st = integers(ends, radius)
    if st is None:
        return None
    H, W = hw
    ax, ay, bx, by, r = st
    # a covered centre 2x + 1 lies within r of the segment: min - r <= 2x + 1 <= max + r
    x0, x1 = max(0, -(-(min(ax, bx) - r - 1) // 2)), min(W - 1, (max(ax, bx) + r - 1) // 2)
    y0, y1 = max(0, -(-(min(ay, by) - r - 1) // 2)), min(H - 1, (max(ay, by) + r - 1) // 2)
    if x0 > x1 or y0 > y1:
        return None
    px = (2 * np.arange(x0, x1 + 1, dtype=np.int64) + 1)[None, :]
    py = (2 * np.arange(y0, y1 + 1, dtype=np.int64) + 1)[:, None]
    dx, dy = bx - ax, by - ay
    vx, vy = px - ax, py - ay                       # (below 2^18: every int64 product here is below 2^37)
    l2, s = dx * dx + dy * dy, vx * dx + vy * dy
    first = (s <= 0) & (vx * vx + vy * vy <= r * r)
    second = (s >= l2) & ((px - bx) ** 2 + (py - by) ** 2 <= r * r)
    cross = np.abs(vx * dy - vy * dx).astype(object)
    third = (s > 0) & (s < l2) & (cross * cross <= r * r * l2).astype(bool)
    mask = first | second | third
    return (y0, x0, mask) if mask.any() else None


def paint(canvas, ends, colour, radius):
    """The strokes in list order over `canvas` (H, W, 3) uint8, in place -> canvas.  Nothing else is touched."""
    for k in range(len(radius)):
        w = covered(canvas.shape[:2], ends[k], radius[k])
        if w is not None:
            y0, x0, mask = w
            canvas[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]][mask] = rgb_bytes(int(colour[k]) & 0xFFFFFF)
    return canvas


# ---------------------------------------------------------------------------------------------------------------------
# the window: one launch of canvases that between them hold the cases of the issue
# ---------------------------------------------------------------------------------------------------------------------
def _filler(rng, n, H, W):
    """short strokes all over the canvas and a little beyond, a fifth of them discs, radii 0 (skipped), 1, 2, 3 and 6"""
    ends = np.empty((n, 4), dtype=np.float32)
    ends[:, 0] = rng.uniform(-10, W + 10, n)
    ends[:, 1] = rng.uniform(-10, H + 10, n)
    ends[:, 2] = ends[:, 0] + rng.uniform(-25, 25, n)
    ends[:, 3] = ends[:, 1] + rng.uniform(-12, 12, n)
    discs = rng.rand(n) < 0.2
    ends[discs, 2:] = ends[discs, :2]
    return ends, rng.randint(0, 1 << 24, n).astype(np.int32), rng.choice(np.array([0, 1, 1, 2, 2, 3, 6]), n).astype(np.int32)


def special_strokes(H, W):
    """the strokes of the issue for an H x W canvas -> list of ((ax, ay, bx, by), colour, radius)"""
    nan, inf = float('nan'), float('inf')
    s = []
    # wholly outside on each of the four sides, nearer than and farther than the radius; crossing each border and each corner
    for e in ((-30, 2, -9, 6), (W + 9, 2, W + 30, 5), (3, -30, 9, -8), (3, H + 8, 9, H + 30), (-2.5, 3, -1.5, 3), (W + 1.2, 3, W + 1.2, 3),
              (-6, 2, 5, 6), (W - 4, 1, W + 6, 5), (10, -5, 14, 3), (10, H - 2, 16, H + 5),
              (-3, -3, 3, 3), (W - 2, -2, W + 4, 3), (-3, H + 3, 2, H - 3), (W - 3, H - 2, W + 3, H + 2)):
        s.append((e, 0x102030, 3))
    # not finite: skipped; radius 0 and below: skipped
    for e in ((nan, 1, 5, 5), (1, nan, 5, 5), (1, 1, inf, 5), (1, 1, 5, -inf), (-inf, -inf, inf, inf), (inf, 1, 5, 5)):
        s.append((e, 0xFF00FF, 2))
    for r in (0, -1, -2 ** 31):
        s.append(((1, 1, 9, 4), 0x00FFFF, r))
    # radii 1, 2, 6, 64 and beyond (clamped to 64); discs; ends at half and quarter pixels
    for k, r in enumerate((1, 2, 6)):
        s.append(((20 + 9 * k, 2.5, 26 + 9 * k, 7.5), 0x0000FF + (k << 12), r))
        s.append(((20.5 + 9 * k, 12.25, 20.5 + 9 * k, 12.25), 0x00FF00 + k, r))
    s.append(((W * 0.5, H * 0.5, W * 0.5 + 3, H * 0.5), 0x404040, 64))
    s.append(((W * 0.5 + 40, H * 0.5, W * 0.5 + 40, H * 0.5), 0x505050, 1000))
    s.append(((W * 0.5 + 40, H * 0.5, W * 0.5 + 40, H * 0.5), 0x606060, 2 ** 31 - 1))
    # ends at +-1e9: clamped to -32768 and 32767 -- a whole row, a whole column, the clamped diagonal
    s.append(((-1e9, 5.5, 1e9, 5.5), 0xAA0000, 1))
    s.append(((7.5, 1e9, 7.5, -1e9), 0x00AA00, 2))
    s.append(((-1e9, -1e9, 1e9, 1e9), 0x0000AA, 2))
    # a diagonal across every tile, and the anti-diagonal
    s.append(((0, 0, W, H), 0xC0C000, 2))
    s.append(((W, 0, 0, H), 0x00C0C0, 1))
    # overlapping strokes in both list orders: a cross, and the same cross a few pixels on with its strokes swapped
    s.append(((40, 3, 52, 9), 0xF00000, 3))
    s.append(((40, 9, 52, 3), 0x00F000, 3))
    s.append(((55, 9, 67, 3), 0x00F000, 3))
    s.append(((55, 3, 67, 9), 0xF00000, 3))
    return s


def _arrays(strokes):
    ends = np.array([e for e, _, _ in strokes], dtype=np.float32).reshape(-1, 4)
    return ends, np.array([c for _, c, _ in strokes], dtype=np.int64).astype(np.int32), np.array([max(r, -2 ** 31) for _, _, r in strokes], dtype=np.int64).astype(np.int32)


def _padded(rng, strokes, n, H, W):
    """`strokes` spread through n - len(strokes) random ones, their own order kept"""
    arrays = _arrays(strokes)
    filler = _filler(rng, n - len(strokes), H, W)
    at = np.sort(rng.choice(n, len(strokes), replace=False))
    rest = np.setdiff1d(np.arange(n), at)
    out = [np.empty((n, 4), dtype=np.float32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)]
    for o, a, f in zip(out, arrays, filler):
        o[at], o[rest] = a, f
    return tuple(out)


def window(seed=23):
    """-> list of canvases, dicts {hw, ends, colour, radius}: sizes 1x1, 3x5, 16x64 (one tile), 17x65 (one pixel over), 130x200, 1x32768
    and 32768x1; stroke counts 0, 1, 255, 256, 600, 257 and 5."""
    rng = np.random.RandomState(seed)
    cs = []

    def add(hw, arrays):
        cs.append(dict(hw=hw, ends=arrays[0], colour=arrays[1], radius=arrays[2]))

    add((1, 1), _arrays([]))
    add((3, 5), _arrays([((2.5, 1.5, 2.5, 1.5), 0x123456, 2)]))                             # one disc: a plus of five pixels
    add((16, 64), _padded(rng, special_strokes(16, 64)[:30], 255, 16, 64))
    add((17, 65), _padded(rng, special_strokes(17, 65), 256, 17, 65))
    add((130, 200), _padded(rng, special_strokes(130, 200), 600, 130, 200))
    # 1 x 32768: the whole row first, then 256 discs stacked on the pixel past the first tile's edge: the last one wins
    row = [((-1e9, 0.5, 1e9, 0.5), 0x0A0B0C, 1)] + [((64.5, 0.5, 64.5, 0.5), (k * 2654435761) & 0xFFFFFF, 1 + k % 3) for k in range(256)]
    add((1, 32768), _arrays(row))
    # 32768 x 1: the whole column, a part of it, discs on the first and the last pixel, one stroke beside the canvas
    col = [((0.5, -1e9, 0.5, 1e9), 0x0C0B0A, 1), ((0.5, 100.2, 0.5, 5000.7), 0xABCDEF, 1), ((0.5, 0.5, 0.5, 0.5), 0x111111, 2),
           ((0.5, 32767.5, 0.5, 32767.5), 0x222222, 64), ((3.0, 10, 3.0, 20000), 0x333333, 4)]
    add((32768, 1), _arrays(col))
    return cs


def tiles(h, w):
    return -(-h // TILE_H) * -(-w // TILE_W)


def tables(cs, only=None, align=1):
    """The launch's arrays: -> dict of numpy arrays `canvases` (C, 6) int64, `ends` (n, 4) float32, `colour`, `radius` (n,) int32, and
    `total_tiles`, `out_bytes`, `spans` [(offset, H, W)].  align: the canvases' byte alignment in the output (1: back to back, so that
    most rows start at odd addresses)."""
    cs = cs if only is None else [cs[c] for c in only]
    table, spans, tile, out, k = [], [], 0, 0, 0
    for c in cs:
        H, W = c['hw']
        out = -(-out // align) * align
        n = len(c['radius'])
        table.append((tile, out, H, W, k, k + n))
        spans.append((out, H, W))
        tile, out, k = tile + tiles(H, W), out + H * W * 3, k + n
    cat = lambda name, dt, shape: np.concatenate([c[name] for c in cs]).astype(dt).reshape(shape)
    return dict(canvases=np.array(table, dtype=np.int64).reshape(-1, COLS), total_tiles=tile, out_bytes=out, spans=spans,
                ends=cat('ends', np.float32, (-1, 4)), colour=cat('colour', np.int32, -1), radius=cat('radius', np.int32, -1))


def run_model(cs, t, flat, only=None):
    """`flat`: the launch's output buffer before the launch (uint8, t['out_bytes']) -> what it holds after, by the model"""
    cs = cs if only is None else [cs[c] for c in only]
    want = flat.copy()
    for c, (off, h, w) in zip(cs, t['spans']):
        img = want[off:off + h * w * 3].reshape(h, w, 3)            # (a view: painted in place)
        paint(img, c['ends'], c['colour'], c['radius'])
    return want
