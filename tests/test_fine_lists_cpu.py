"""The fine work-list modes on the host: the plain-Python model of tests/fine_lists.py (modes 4 and 5 of `cvpce_skip_layer.skip`) against
the properties include/cvpce_amd.h states, against the model of modes 2 and 3 (tests/footprint.py worklist_model), and the S = 64
construction that tests/test_gpu_skip_fine.py runs single layers on."""
import random

import fine_lists as fl
import footprint as fp

# the embedder's twelve layers at S = 256 (`skip_plan(256)`: stem, conv2_1 .. conv5_3) and the op chain of VGG16 'D' up to relu5_3
S256, MASK256 = 256, sum(1 << i for i in (2, 5, 9, 13))
PLAN256 = [[128, 128, 8, 8, 3, 256, 256, 0, 1], [128, 128, 16, 32, 4, 128, 128, 3, 2], [64, 64, 8, 16, 6, 128, 128, 4, 2],
           [64, 64, 16, 16, 7, 64, 64, 6, 3], [64, 64, 16, 16, 8, 64, 64, 7, 3], [32, 32, 8, 8, 10, 64, 64, 8, 3],
           [32, 32, 16, 16, 11, 32, 32, 10, 3], [32, 32, 16, 16, 12, 32, 32, 11, 3], [16, 16, 8, 8, 14, 32, 32, 12, 3],
           [16, 16, 16, 16, 15, 16, 16, 14, 3], [16, 16, 16, 16, 16, 16, 16, 15, 3], [16, 16, 16, 16, 17, 16, 16, 16, 3]]
FINE = {2: 4, 3: 5}


def _extents(n, seed):
    r = random.Random(seed)
    ext = [[r.randint(1, S256), S256] if i % 3 else [S256, r.randint(1, S256)] for i in range(n)]
    ext[5:9] = [[S256, S256], [0, 0], [1, S256], [S256, 255]]
    return ext + [[S256, S256]]


def _fields(e):
    return (e >> 56) & 0xFF, (e >> 16) & 0xFFFF, (e >> 8) & 0xFF, e & 0xFF           # rows, crop, ty, tx


def test_modes_up_to_3_are_the_existing_model():
    """on modes 0 .. 3 the model is tests/footprint.py's, entry for entry (and its thin lists are empty)"""
    ext = _extents(131, 3)
    for mode in (0, 1, 2, 3):
        layers = [l[:-1] + [min(l[-1], mode)] for l in PLAN256]
        new, old = fl.model(ext, S256, MASK256, layers), fp.worklist_model(ext, S256, MASK256, layers)
        for (want, swant, twant, work, comp), o in zip(new, old):
            assert (want, swant, work, comp) == o and twant == []


def test_fine_modes_against_modes_2_and_3():
    ext = _extents(131, 3)
    fine = [l[:-1] + [FINE.get(l[-1], l[-1])] for l in PLAN256]
    coarse_t = [fl.tiles(ext, S256, MASK256, l) for l in PLAN256]
    classes = {fl.STRIP: 0, fl.THIN: 0}
    for li, (layer, (want, swant, twant, work, comp)) in enumerate(zip(fine, fl.model(ext, S256, MASK256, fine))):
        h, w, th, tw, out_ops, ih, iw, in_ops, skip = layer
        per_crop = fl.tiles(ext, S256, MASK256, layer)
        total = 0
        for c, (crop, coarse) in enumerate(zip(per_crop, coarse_t[li])):
            # no list loses a tile that modes 2 / 3 list, and no tile computes more rows than there
            assert [(ty, tx) for ty, tx, _, _ in crop] == [(ty, tx) for ty, tx, _, _ in coarse], (li, c)
            eoy = fl.extent(ext[c][0], S256, MASK256, out_ops, h)
            for (ty, tx, rows, cls), (_, _, crows, _) in zip(crop, coarse):
                need = fl.needed_rows(min(th, eoy - ty * th), th)
                assert rows % 2 == 0 and 2 <= rows <= 16 and need <= rows <= crows and (skip < 4 or rows - need < 2), (li, c, ty, rows, need)
                # the thin and strip classes partition the last-row tiles with rows <= 4 (mode 5; mode 4 has no strip class)
                last = ty == crop[-1][0]
                assert cls == ((fl.THIN if rows == 2 else fl.STRIP) if (skip == 5 and last and rows <= 4) else fl.MAIN), (li, c, ty, rows, cls)
                if cls != fl.MAIN:
                    classes[cls] += 1
                total += 4 if cls == fl.STRIP else (2 if cls == fl.THIN else (rows + 1 if rows < 16 else 16))
            # `computed`: whole tile rows and the last one's rows -- what cvpce_mac_init covers the rest of
            assert comp[c] == ([(crop[-1][0]) * 16 + crop[-1][2], len({tx for _, tx, _, _ in crop})] if crop else [0, 0])
        # the work figure: rows + 1 sixteenths for a cut tile, 16 for a full one, 4 per strip, 2 per thin strip
        assert work == total, li
        ent = want + swant + twant
        assert len(ent) == len(set(ent)) == sum(len(c) for c in per_crop)
        assert all(_fields(e)[0] == 4 for e in swant) and all(_fields(e)[0] == 2 for e in twant)
        for lst in (want, swant, twant):                         # crop-major, row-major inside a crop
            assert [_fields(e)[1:] for e in lst] == sorted(_fields(e)[1:] for e in lst)
        if skip != 5:
            assert not swant and not twant
    assert classes[fl.STRIP] > 0 and classes[fl.THIN] > 0


def test_work_never_exceeds_the_coarse_modes():
    ext = _extents(131, 7)
    fine = [l[:-1] + [FINE.get(l[-1], l[-1])] for l in PLAN256]
    for (_, _, _, work, _), (_, _, cwork, _) in zip(fl.model(ext, S256, MASK256, fine), fp.worklist_model(ext, S256, MASK256, PLAN256)):
        assert work <= cwork


def test_s64_construction():
    """per tested layer every even `rows` 2 .. 16; both strip classes non-empty on the mode-5 layers, a thin count that is no multiple
    of 4, thin strips of different crops in one pass of four; at most 24 crops"""
    assert len(fl.EXT) <= 24 and fl.N == len(fl.EXT) + 1
    assert [l[-1] for l in fl.LAYERS] == [1, 4, 5, 5]
    m = fl.construction()
    for li in (1, 2, 3):
        want, swant, twant, _, _ = m[li]
        assert {_fields(e)[0] for e in want + swant + twant} == set(range(2, 17, 2)), li
        if fl.LAYERS[li][-1] == 5:
            assert swant and twant and len(twant) % 4 != 0, li
            assert len(swant) % 3 != 0                           # the last strip pass repeats an entry
            passes = [twant[i:i + 4] for i in range(0, len(twant), 4)]
            assert any(len({_fields(e)[1] for e in p}) > 1 for p in passes), li
        else:
            assert not swant and not twant
    # a crop without a content column still lists one tile column behind the stem (every conv grows the extent by one); the full crop
    # and the constant crop list every tile whole
    empty = next(c for c, e in enumerate(fl.EXT) if e[1] == 0)
    for li in (1, 2, 3):
        h, w, th, tw = fl.LAYERS[li][:4]
        ents = m[li][0] + m[li][1] + m[li][2]
        assert {_fields(e)[3] for e in ents if _fields(e)[1] == empty} == {0}
        for c in (fl.EXT.index([fl.S, fl.S]), fl.N - 1):
            mine = [e for e in ents if _fields(e)[1] == c]
            assert len(mine) == -(-h // th) * -(-w // tw) and all(_fields(e)[0] == 16 for e in mine)
