"""Plain-Python restatement of the matcher's launch decision as cvpce_match_topk made it before csrc/match.hip got match_plan (its inline
cost model, match_small_tq and match_large_k_plan): the same operations in the same order on Python floats (IEEE doubles, like the C
code), strict `<` in the same loop order, so ties resolve alike.  tests/test_match_plan_cpu.py compares cvpce_match_plan with it."""
FIELDS = ('path', 'tq', 'nq', 'mg', 'tiles_g', 'tiles_q', 'lds', 'threads', 'chunk', 'gpad', 'chunk_bytes', 'workspace')
LDS = {('f32', 128, False): 2 * 2 * 128 * 256, ('f32', 128, True): 2 * 2 * 128 * 256, ('bf16', 128, False): 128 * 128 * 4 + 2048 + 512,
       ('bf16', 64, False): 2 * (128 + 64) * 128, ('bf16', 64, True): 2 * (128 + 64) * 128, ('bf16', 128, True): 128 * 129 * 4 + 512}


def small_tq(tiles_g, qn, cus=256):
    t128, t64 = tiles_g * ((qn + 127) // 128), tiles_g * ((qn + 63) // 64)
    c128, c64 = float((t128 + 2 * cus - 1) // (2 * cus)) * 1.0, float((t64 + 3 * cus - 1) // (3 * cus)) * 0.6
    return 64 if c64 < c128 else 128


def large_k(qn, gn, k):
    gpad = (gn + 127) // 128 * 128
    nsurv = 2 if k > 16384 else 1
    qc = (256 << 20) // (gpad * 4 + k * 8 * nsurv)
    if qc >= 128:
        qc = qc // 128 * 128
    qc = min(max(qc, 1), qn)
    return qc, gpad, (qc * gpad * 4 + 255) // 256 * 256 + nsurv * ((qc * k * 8 + 255) // 256 * 256)


def plan(qn, gn, d, k, f32, forced=(0, 0, 0), cus=256):
    """-> dict of FIELDS, or None where the arguments are rejected"""
    es = 4 if f32 else 2
    if d <= 0 or d % 64 or k < 1 or gn < k or (gn + 128) * d * es >= 1 << 32 or (qn + 128) * d * es >= 1 << 32:
        return None
    core, fnq, fmg = forced
    tiles_g = (gn + 127) // 128
    if k > 16:
        qc, gpad, nbytes = large_k(qn, gn, k)
        tq = 128 if f32 else small_tq(tiles_g, qc, cus)
        return dict(zip(FIELDS, (2, tq, 0, 0, tiles_g, (qc + tq - 1) // tq, LDS['f32' if f32 else 'bf16', tq, True], 256, qc, gpad, nbytes, nbytes + 512)))
    ws = qn * tiles_g * k * 8 + 512
    tq = 128 if f32 else small_tq(tiles_g, qn, cus)
    big_nq, big_mg = 0, 2
    if not f32:
        dk = d / 512.0
        t128, t64 = tiles_g * ((qn + 127) // 128), tiles_g * ((qn + 63) // 64)
        r128, r64 = (t128 + 2 * cus - 1) // (2 * cus), (t64 + 3 * cus - 1) // (3 * cus)
        e128 = 10.4 + float(r128) * dk * 9.0 * (1.0 + 0.75 * float(t128) / float(r128 * 2 * cus))
        e64 = 10.4 + float(r64) * dk * 5.4 * (1.0 + 0.75 * float(t64) / float(r64 * 3 * cus))
        best, best_big = (e64 if e64 < e128 else e128), 1e30
        for mg in (1, 2):
            for nq in (2, 3, 4, 5):
                if (fnq and nq != fnq) or (fmg and mg != fmg) or (mg == 1 and nq == 5):
                    continue
                t = ((gn + 128 * mg - 1) // (128 * mg)) * ((qn + 64 * nq - 1) // (64 * nq))
                rounds = (t + cus - 1) // cus
                u = float(t) / float(rounds * cus)
                e = 3.9 + 0.48 * nq + float(rounds) * dk * (0.74 + 1.97 * nq) * (0.575 if mg == 1 else 1.0) * (1.0 + 0.75 * u)
                if e < best_big:
                    best_big, big_nq, big_mg = e, nq, mg
        if core == 1 or (core == 0 and (not best_big < best or qn * gn < 64 * 1024)):
            big_nq = 0
    if big_nq:
        tg = 128 * big_mg
        if (qn + 64 * big_nq) * d * 2 >= 1 << 32 or (gn + tg) * d * 2 >= 1 << 32:
            return None
        return dict(zip(FIELDS, (1, 0, big_nq, big_mg, (gn + tg - 1) // tg, (qn + 64 * big_nq - 1) // (64 * big_nq),
                                 2 * (tg + 64 * big_nq) * 128, 512, 0, 0, 0, ws)))
    return dict(zip(FIELDS, (0, tq, 0, 0, tiles_g, (qn + tq - 1) // tq, LDS['f32' if f32 else 'bf16', tq, False], 256, 0, 0, 0, ws)))
