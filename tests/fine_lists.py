"""The FINE work-list modes of include/cvpce_amd.h (`cvpce_skip_layer.skip` 4 and 5) in plain Python, independent of the kernel, and
the S = 64 construction the GPU test of the fine lists runs single layers on.  (Not a test module: test_fine_lists_cpu.py checks the
model and the construction on the host, test_gpu_skip_fine.py holds csrc/skiplist.hip and the halo kernels to them.)

Mode 4 is mode 2 and mode 5 is mode 3 with a tile's `rows` -- its conv-output rows that are not wholly constant -- rounded up to 2
instead of 4.  Mode 5 has two strip classes: last-row tiles with rows == 4 (the strip list, three to a pass) and with rows == 2 (the
THIN strip list, four to a pass)."""

MAIN, STRIP, THIN = 0, 1, 2


def extent(e0, size, pool_mask, nops, dim):
    """a crop's content extent through the first `nops` ops of the pass: a conv grows it by 1, a pool halves it upwards"""
    if e0 >= size:
        return dim
    e = e0
    for i in range(nops):
        e = (e + 1) // 2 if (pool_mask >> i) & 1 else e + 1
    return min(dim, e)


def tile_rows(act, th, skip):
    """`rows` of a last listed tile row with `act` of its th output rows not constant: sixteenths of the tile, rounded up to 4 | 2"""
    r = -(-act * 16 // th)
    step = 2 if skip >= 4 else 4
    return min(16, -(-r // step) * step)


def needed_rows(act, th):
    """the conv-output rows (before a fused pool) of a tile that are not constant"""
    return min(16, -(-act * 16 // th))


def tiles(ext, size, pool_mask, layer):
    """per crop: [(ty, tx, rows, class)] of its listed tiles in list order, class MAIN | STRIP | THIN, for any mode 0 .. 5"""
    h, w, th, tw, out_ops, ih, iw, in_ops, skip = layer
    ty_n, tx_n = -(-h // th), -(-w // tw)
    out = []
    for ey0, ex0 in ext:
        ny, nx = ty_n, tx_n
        if skip:
            ny = min(ty_n, -(-extent(ey0, size, pool_mask, out_ops, h) // th))
            nx = min(tx_n, -(-extent(ex0, size, pool_mask, out_ops, w) // tw))
        if nx == 0:
            ny = 0
        crop = []
        for ty in range(ny):
            rows, cls = 16, MAIN
            if skip >= 2 and ty == ny - 1:
                rows = tile_rows(min(th, extent(ey0, size, pool_mask, out_ops, h) - ty * th), th, skip)
                if skip in (3, 5) and rows == 4:
                    cls = STRIP
                elif skip == 5 and rows == 2:
                    cls = THIN
            crop += [(ty, tx, rows, cls) for tx in range(nx)]
        out.append(crop)
    return out


def model(ext, size, pool_mask, layers):
    """ext: (rows, cols) per crop, the constant crop included -> per layer (list entries, strip-list entries, thin-strip entries, MFMA
    work in sixteenths of a tile, [conv rows computed, tile columns listed] per crop): what cvpce_embed_worklists writes"""
    res = []
    for layer in layers:
        h, w, th, tw, out_ops, ih, iw, in_ops, skip = layer
        lists, work, comp = ([], [], []), 0, []
        for c, ((ey0, ex0), crop) in enumerate(zip(ext, tiles(ext, size, pool_mask, layer))):
            ext_in = (extent(ey0, size, pool_mask, in_ops, ih) << 12) | extent(ex0, size, pool_mask, in_ops, iw)
            for ty, tx, rows, cls in crop:
                lists[cls].append((((rows << 24) | ext_in) << 32) | (c << 16) | (ty << 8) | tx)
                work += 4 if cls == STRIP else (2 if cls == THIN else (rows + 1 if rows < 16 else 16))
            if crop:
                ny = crop[-1][0] + 1
                comp.append([(ny - 1) * 16 + crop[-1][2], len([t for t in crop if t[0] == 0])])
            else:
                comp.append([0, 0])
        res.append((lists[MAIN], lists[STRIP], lists[THIN], work, comp))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# the S = 64 construction of tests/test_gpu_skip_fine.py: the layers of tests/exact_cases.py WL_LAYERS in the fine modes, and crops whose
# extents produce every even `rows` the layers' maps allow
# ---------------------------------------------------------------------------------------------------------------------------------
S, POOL_MASK = 64, 0b0100100
#   stem (whole tiles) | halo3 list 64 -> 128 on 32 x 32 | halo2 list, fused pool, 128 -> 256 on 32 x 32 | halo2 list + strips + thin, 256 -> 264 on 32 x 32
# (layers 2 and 3 both read the tensor named 4; a 16 x 16 map behind the pool could not show rows == 2: its extent is at least 4)
LAYERS = [[32, 32, 8, 8, 3, 64, 64, 0, 1], [32, 32, 16, 32, 4, 32, 32, 3, 4], [16, 16, 8, 8, 6, 32, 32, 4, 5], [32, 32, 16, 16, 5, 32, 32, 4, 5]]
CONVS = {1: (64, 128, 32, False), 2: (128, 256, 32, True), 3: (256, 264, 32, False)}      # layer -> cin, cout, input size, fused pool
# (rows, cols) of the crops' content at S = 64; the constant crop follows them.  The row extents 3, 7 .. 27, 29 take the last listed
# tile row of every layer through every even `rows` 2 .. 16 (chosen with `model`: test_fine_lists_cpu.py); narrow crops (cols 20, 9)
# list one tile column where the others list two, so the thin strips of one pass come from different crops and the thin counts are no
# multiples of 4; a full crop and one without a content column complete the set.
EXT = [[3, 64], [7, 64], [11, 64], [15, 64], [19, 64], [23, 64], [27, 64], [29, 64], [27, 20], [28, 9], [31, 20], [25, 64], [64, 64], [9, 0]]
N = len(EXT) + 1


def construction():
    """model(...) of the S = 64 construction, the constant crop last"""
    return model(EXT + [[S, S]], S, POOL_MASK, LAYERS)
