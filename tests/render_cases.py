"""The picture rule of DESIGN.md 4b in plain numpy, and the cases the compositor is tested on.  (Not a test module:
test_render_cpu.py pins the model on the host, test_gpu_render.py compares csrc/render.hip with it byte for byte.)

The model paints FORWARD: item after item in list order, each over what is there -- the kernel searches backward from the last item
and stops at the first hit, so the two share the rule and nothing of its evaluation.
"""
import numpy as np

TILE_W, TILE_H, CHUNK = 64, 16, 256
COLS = 10
SRC_NONE, SRC_BASE = -1, -2
MAX_SIDE = 32768
BACKGROUND = 0xC8E6FA


def rgb_bytes(colour):
    return np.array([colour & 255, (colour >> 8) & 255, (colour >> 16) & 255], dtype=np.uint8)


def extents(box):
    """box: 4 float32 -> (X1, Y1, bw, bh) or None where the item is skipped"""
    b = np.asarray(box, dtype=np.float32)
    if not np.isfinite(b).all():
        return None
    b = np.clip(b, np.float32(-32768), np.float32(32767))
    x1, y1, x2, y2 = int(np.floor(b[0])), int(np.floor(b[1])), int(np.ceil(b[2])), int(np.ceil(b[3]))
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2 - x1, y2 - y1


def axis(i, b, s):
    """pixels i (int64 array) of a box side b -> (p0, p1, f) of a source side s; Python-exact integers through int64 (the largest
    numerator is 131071 * 32768 * 256 < 2^41)"""
    i = np.asarray(i, dtype=np.int64)
    px = np.clip(((2 * i + 1) * s * 256) // (2 * b) - 128, 0, (s - 1) * 256)
    p0 = px >> 8
    return p0, np.minimum(p0 + 1, s - 1), px & 255


def sample(source, bw, bh, ii, jj):
    """source (sh, sw, 3) uint8 resampled to a bw x bh box, at the box pixels jj x ii -> (len(jj), len(ii), 3) uint8"""
    sh, sw = source.shape[:2]
    x0, x1, fx = axis(ii, bw, sw)
    y0, y1, fy = axis(jj, bh, sh)
    s = source.astype(np.int64)
    fx, fy = fx[None, :, None], fy[:, None, None]
    v = ((256 - fx) * (256 - fy) * s[y0][:, x0] + fx * (256 - fy) * s[y0][:, x1] + (256 - fx) * fy * s[y1][:, x0] + fx * fy * s[y1][:, x1] + 32768) >> 16
    return v.astype(np.uint8)


def resample(source, bh, bw):
    """the whole source at bh x bw"""
    return sample(source, bw, bh, np.arange(bw), np.arange(bh))


def paint(hw, box, src, colour, thickness, atlas, base=None, background=BACKGROUND):
    """One canvas: the items in list order over the background.  atlas: list of (h, w, 3) uint8 arrays; base: (h, w, 3) uint8 or None."""
    H, W = hw
    canvas = np.empty((H, W, 3), dtype=np.uint8)
    canvas[:] = rgb_bytes(background)
    for k in range(len(src)):
        e = extents(box[k])
        if e is None:
            continue
        X1, Y1, bw, bh = e
        i0, i1, j0, j1 = max(0, -X1), min(bw, W - X1), max(0, -Y1), min(bh, H - Y1)
        if i0 >= i1 or j0 >= j1:
            continue
        ii, jj = np.arange(i0, i1, dtype=np.int64), np.arange(j0, j1, dtype=np.int64)
        t = int(thickness[k])
        edge = np.minimum(np.minimum(ii, bw - 1 - ii)[None, :], np.minimum(jj, bh - 1 - jj)[:, None])
        ring = (edge < t) if t >= 1 else np.zeros(edge.shape, dtype=bool)
        s = int(src[k])
        source = base if s == SRC_BASE else (atlas[s] if 0 <= s < len(atlas) else None)
        region = canvas[Y1 + j0:Y1 + j1, X1 + i0:X1 + i1]
        if source is not None:
            region[:] = sample(source, bw, bh, ii, jj)
        region[ring] = rgb_bytes(int(colour[k]))
    return canvas


# ---------------------------------------------------------------------------------------------------------------------
# the window: one launch of canvases that between them hold the cases of the issue
# ---------------------------------------------------------------------------------------------------------------------
def atlas_images(seed=5):
    """rows 0-3: 1x1, 1x256, 256x1, 256x256 (h x w); 4, 5: small odd sizes.  Random bytes, row 3 half checkerboard."""
    rng = np.random.RandomState(seed)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((1, 1), (1, 256), (256, 1), (256, 256), (12, 9), (30, 41))]
    yy, xx = np.mgrid[:256, :128]
    imgs[3][:, :128] = (((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None]
    return imgs


def _filler(rng, n, H, W, rows):
    box = np.empty((n, 4), dtype=np.float32)
    box[:, 0] = rng.uniform(-12, W + 6, n)
    box[:, 1] = rng.uniform(-12, H + 6, n)
    box[:, 2] = box[:, 0] + rng.uniform(0.2, 30, n)
    box[:, 3] = box[:, 1] + rng.uniform(0.2, 14, n)
    src = rng.choice(np.array([SRC_NONE, SRC_NONE, SRC_BASE] + list(range(rows))), n).astype(np.int32)
    colour = rng.randint(0, 1 << 24, n).astype(np.int32)
    thickness = rng.choice(np.array([0, 0, 1, 2, 5]), n).astype(np.int32)
    return box, src, colour, thickness


def special_items(H, W, rows):
    """the boxes, rings, orderings and bad sources of the issue, for an H x W canvas -> list of (box, src, colour, thickness)"""
    nan, inf = float('nan'), float('inf')
    s = []
    # outside on each of the four sides; straddling each side and each corner
    for b in ((-20, 2, -5, 6), (W + 3, 2, W + 20, 6), (3, -30, 9, -2), (3, H + 1, 9, H + 9),
              (-4, 2, 3, 6), (W - 3, 1, W + 5, 5), (10, -3, 16, 2), (10, H - 2, 16, H + 4),
              (-3, -3, 3, 3), (W - 2, -2, W + 4, 3), (-3, H - 3, 2, H + 3), (W - 3, H - 2, W + 3, H + 2)):
        s.append((b, 4, 0x102030, 1))
    # not finite; zero and negative extents; a width of 0.3; 1-pixel boxes
    for b in ((nan, 1, 5, 5), (1, nan, 5, 5), (1, 1, inf, 5), (1, 1, 5, -inf), (-inf, -inf, inf, inf), (inf, 1, 5, 5)):
        s.append((b, 5, 0xFF00FF, 2))
    for b in ((5, 2, 5, 6), (7, 2, 4, 6), (5, 4, 9, 4), (5, 6, 9, 1)):
        s.append((b, 5, 0x00FFFF, 2))
    s.append(((20.2, 1.0, 20.5, 4.0), 4, 0x334455, 0))              # width 0.3: one pixel column
    s.append(((22.7, 1.0, 23.0, 4.0), SRC_NONE, 0x334455, 1))
    for k, src in enumerate((0, 1, 2, 3, 4, SRC_NONE)):
        s.append(((30 + k, 2, 31 + k, 3), src, 0x0000FF, 1 if src == SRC_NONE else 0))
    # nothing inside above a pasted item: the interior shows through, the ring does not
    s.append(((36, 1, 50, 8), 5, 0, 0))
    s.append(((38, 2, 48, 7), SRC_NONE, 0x00FF00, 2))
    # a ring that is the box (thickness at least half the box); thickness 0 with nothing inside (paints nothing)
    s.append(((40, 3, 46, 6), 4, 0xAA5500, 3))
    s.append(((41, 3, 45, 6), 3, 0x0055AA, 1000))
    s.append(((0, 0, W, H), SRC_NONE, 0xFFFFFF, 0))
    # bad sources: rows, rows + 5, -3 -- each counts as nothing inside
    for k, src in enumerate((rows, rows + 5, -3)):
        s.append(((52 + 3 * k, 1, 56 + 3 * k, 7), src, 0x7F007F, 1))
    return s


def _arrays(items):
    box = np.array([b for b, _, _, _ in items], dtype=np.float32).reshape(-1, 4)
    return box, np.array([v[1] for v in items], dtype=np.int32), np.array([v[2] for v in items], dtype=np.int32), np.array([v[3] for v in items], dtype=np.int32)


def _padded(rng, items, n, H, W, rows):
    """`items` spread through n - len(items) random ones, their own order kept"""
    box, src, colour, thickness = _arrays(items)
    fb, fs, fc, ft = _filler(rng, n - len(items), H, W, rows)
    at = np.sort(rng.choice(n, len(items), replace=False))
    out = [np.empty((n, 4), dtype=np.float32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)]
    rest = np.setdiff1d(np.arange(n), at)
    for o, a, f in zip(out, (box, src, colour, thickness), (fb, fs, fc, ft)):
        o[at], o[rest] = a, f
    return tuple(out)


def window(seed=11):
    """-> dict: 'atlas' (list of images), 'background', 'canvases': list of dicts {hw, base (image or None), box, src, colour, thickness}.
    Canvas sizes 1x1, 5x7, widths 63, 64, 65, 67 and one canvas three tiles high; item counts 0, 1, 255, 256, 257 and 600."""
    rng = np.random.RandomState(seed)
    atlas = atlas_images()
    rows = len(atlas)
    img = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    whole = lambda H, W, src: ((0, 0, W, H), src, 0, 0)
    cs = []

    def add(hw, base, arrays):
        cs.append(dict(hw=hw, base=base, box=arrays[0], src=arrays[1], colour=arrays[2], thickness=arrays[3]))

    add((1, 1), None, _arrays([]))                                                                  # 0 items: the background
    add((5, 7), img(5, 7), _arrays([whole(5, 7, SRC_BASE)]))                                        # 1 item: the base at its own size
    add((9, 63), img(13, 50), _padded(rng, [whole(9, 63, SRC_BASE)] + special_items(9, 63, rows)[:20], 255, 9, 63, rows))     # a base of another size
    add((9, 64), None, _padded(rng, special_items(9, 64, rows) + [whole(9, 64, SRC_BASE)], 256, 9, 64, rows))               # no base, items that ask for one
    # 257 items stacked on one pixel past the first tile's edge: the last wins
    stack = [((64, 3, 65, 4), (k % (rows + 1)) - 1, (k * 2654435761) & 0xFFFFFF, k % 2) for k in range(256)] + [((64, 3, 65, 4), SRC_NONE, 0x123456, 1)]
    add((9, 65), img(9, 65), _arrays(stack))
    add((9, 67), img(20, 20), _padded(rng, special_items(9, 67, rows), 600, 9, 67, rows))
    # three tiles high and wide: every source enlarged about 40 times and reduced to one pixel, whole-canvas and larger boxes, a box wide
    # enough for the 64-bit division (40000 * 256 >= 2^23)
    H, W = 40, 130
    big = [whole(H, W, 4),
           ((-20000, -20000, 20000, 20000), 3, 0, 0),               # larger than the canvas on all sides
           ((-30, -30, 60, 100), SRC_BASE, 0xFF0000, 31),           # the base enlarged, its ring on the canvas's first row and column
           ((100, -4000, 10340, 6240), 3, 0x00FF00, 3),             # 256 x 256 enlarged 40 times, cut on three sides
           ((-5000, 25, 5240, 65), 1, 0, 0), ((50, -3000, 90, 7240), 2, 0, 0),        # 1 x 256 and 256 x 1 enlarged 40 times
           ((2, 2, 42, 42), 0, 0x0000FF, 1), ((100, 5, 140, 45), 0, 0, 0)]            # 1 x 1 enlarged 40 times
    big += [((95 + k, 20, 96 + k, 21), k, 0, 0) for k in range(4)]
    add((H, W), img(64, 64), _arrays(big))
    return dict(atlas=atlas, background=BACKGROUND, canvases=cs)


def run_model(win, only=None):
    """-> the canvases of the window (or of the canvases `only`) as the model paints them"""
    cs = win['canvases'] if only is None else [win['canvases'][c] for c in only]
    return [paint(c['hw'], c['box'], c['src'], c['colour'], c['thickness'], win['atlas'], c['base'], win['background']) for c in cs]


def tiles(h, w):
    return -(-h // TILE_H) * -(-w // TILE_W)


def tables(win, only=None, align=1):
    """The launch's arrays: -> dict of numpy arrays `canvases` (C, 10) int64, `base`, `atlas` flat uint8, `atlas_rows` (rows, 3) int32,
    `box`, `src`, `colour`, `thickness`, and `total_tiles`, `out_bytes`, `spans` [(offset, H, W)].  align: the canvases' byte alignment in
    the output (1: back to back, so that most rows start at odd addresses)."""
    cs = win['canvases'] if only is None else [win['canvases'][c] for c in only]
    rows, off = [], 0
    for im in win['atlas']:
        rows.append((off, im.shape[0], im.shape[1]))
        off += im.size
    table, spans, bases, tile, out, k, b_off = [], [], [], 0, 0, 0, 0
    for c in cs:
        H, W = c['hw']
        out = -(-out // align) * align
        n = len(c['src'])
        if c['base'] is None:
            b = (-1, 0, 0)
        else:
            b = (b_off, c['base'].shape[0], c['base'].shape[1])
            bases.append(c['base'].reshape(-1))
            b_off += c['base'].size
        table.append((tile, out, H, W) + b + (k, k + n, 0))
        spans.append((out, H, W))
        tile, out, k = tile + tiles(H, W), out + H * W * 3, k + n
    cat = lambda name, dt, shape: np.concatenate([c[name] for c in cs]).astype(dt).reshape(shape)
    return dict(canvases=np.array(table, dtype=np.int64).reshape(-1, COLS), total_tiles=tile, out_bytes=out, spans=spans,
                base=np.concatenate(bases) if bases else np.zeros(0, dtype=np.uint8), atlas=np.concatenate([im.reshape(-1) for im in win['atlas']]),
                atlas_rows=np.array(rows, dtype=np.int32).reshape(-1, 3), box=cat('box', np.float32, (-1, 4)), src=cat('src', np.int32, -1),
                colour=cat('colour', np.int32, -1), thickness=cat('thickness', np.int32, -1))
