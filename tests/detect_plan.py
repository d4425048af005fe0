"""Plain-Python restatement of the launch decision of the detector's post-processing as cvpce_detect_postprocess, launch_postprocess and
cvpce_detect_workspace_bytes made it before csrc/detect.hip got detect_plan: the argument checks in their order, the chunk list, the two
fallbacks to the one-kernel decode and the switch, the dynamic LDS of nms_sort, the phase-1 limit, and the workspace as the carve laid it
out (mask first, every sub-allocation rounded up to 256 bytes) and as the query summed it.  tests/test_detect_plan_cpu.py compares
cvpce_detect_plan with it."""
import os

MAX_LEVELS, DECODE_CHUNK, DECODE_MAX_RUNS, DECODE_RUNS_PER_LEVEL = 8, 8192, 32, 12
PARTS = ('mask', 'cand_boxes', 'cand_scores', 'cand_logits', 'cand_labels', 'cand_count', 's_boxes', 's_scores', 's_labels', 's_off', 's_total',
         'runs', 'done')
FIELDS = ('cap', 'chunked', 'why', 'chunks') + tuple(f'chunk_first{l}' for l in range(MAX_LEVELS + 1)) + (
    'Tmax', 'words', 'sort_lds', 'limit', 'launches', 'workspace') + tuple('off_' + p for p in PARTS)
CHUNKED, MERGE_LIMIT, WORKSPACE_ROOM, SWITCH = 0, 1, 2, 3


def query(grids, n, a, k, topk, dpi):
    """cvpce_detect_plan -> (return code, dict of FIELDS)"""
    import ctypes
    from cvpce_amd._lib import lib
    gh = (ctypes.c_int * max(len(grids), 1))(*[g[0] for g in grids])
    gw = (ctypes.c_int * max(len(grids), 1))(*[g[1] for g in grids])
    out = (ctypes.c_longlong * len(FIELDS))()
    rc = lib.cvpce_detect_plan(gh, gw, len(grids), n, a, k, topk, dpi, out)
    return rc, dict(zip(FIELDS, out))


def capacity(topk):
    return 1024 if topk <= 1024 else 4096 if topk <= 4096 else 0


def workspace_bytes(n, L, topk):
    """cvpce_detect_workspace_bytes"""
    slot = L * topk
    tmax = (slot + 63) // 64 * 64
    words = tmax // 64
    cap = capacity(topk) or 1024
    b = n * slot * (4 + 1 + 1 + 1) * 4
    b += n * L * 4
    b += n * tmax * (4 + 1 + 1 + 1) * 4
    b += n * 4
    b += n * tmax * words * 8
    b += n * L * DECODE_RUNS_PER_LEVEL * cap * 8
    b += n * 4
    return b + 16 * 256


def carve(n, L, topk, cap):
    """the sub-allocations in the order cvpce_detect_postprocess took them -> [(offset, bytes)]"""
    slot = L * topk
    tmax = (slot + 63) // 64 * 64
    words = tmax // 64
    sizes = [n * tmax * words * 8, n * slot * 16, n * slot * 4, n * slot * 4, n * slot * 4, n * L * 4, n * tmax * 16, n * tmax * 4, n * tmax * 4,
             n * tmax * 4, n * 4, n * L * DECODE_RUNS_PER_LEVEL * cap * 8, n * 4]
    out, p = [], 0
    for s in sizes:
        out.append((p, s))
        p += (s + 255) // 256 * 256
    return out


def plan(grids, n, a, k, topk, dpi):
    """-> dict of FIELDS, or None where the arguments are rejected (n >= 1)"""
    L = len(grids)
    cap = capacity(topk)
    if L < 1 or L > MAX_LEVELS or a < 1 or k < 1 or topk < 1 or cap == 0 or dpi < 1:
        return None
    sort_cap = 8192 if cap == 1024 else 20480
    if L * topk > sort_cap or dpi > sort_cap:
        return None
    slot = L * topk
    tmax = (slot + 63) // 64 * 64
    words = tmax // 64
    max_runs = L * DECODE_RUNS_PER_LEVEL
    max_merge = DECODE_MAX_RUNS * 1024 // cap
    why, chunks, first = CHUNKED, 0, []
    for gh, gw in grids:
        if gh < 1 or gw < 1:
            return None
        nl = gh * gw * a * k
        nch = (nl + DECODE_CHUNK - 1) // DECODE_CHUNK
        if nl > 0x7FFFFFFF:
            return None
        if nch > max_merge:
            why = MERGE_LIMIT
        first.append(chunks)
        chunks += min(nch, max_merge)
    first.append(chunks)
    if why == CHUNKED and chunks > max_runs:
        why = WORKSPACE_ROOM
    if why == CHUNKED and os.environ.get('CVPCE_DECODE_ONE_KERNEL') is not None:
        why = SWITCH
    sort_lds = L * (1024 if cap == 1024 else topk) * 4
    limit = dpi * 8
    limit = (max(limit, 1024) + 63) // 64 * 64
    if limit >= tmax or os.environ.get('CVPCE_NMS_ONE_PHASE') is not None:
        limit = 0
    launches = (2 if why == CHUNKED else 1) + 1 + (4 if limit else 2)
    first += [0] * (MAX_LEVELS + 1 - len(first))
    return dict(zip(FIELDS, [cap, int(why == CHUNKED), why, chunks] + first + [tmax, words, sort_lds, limit, launches, workspace_bytes(n, L, topk)]
                    + [o for o, _ in carve(n, L, topk, cap)]))
