"""Timing of the matcher's large-k path (k > 16: distance block -> select -> sort) beside the fused k <= 16 path, on one GPU.

For every (shape, dtype, k): warm-up, then the median over several timed windows (HIP events around a window of calls, then a
synchronise) of one `cvpce_match_topk` call with its buffers allocated up front.  Beside it, as a timing yardstick only (not a
parity check): torch.mm + torch.topk(sorted=True) on the same operands.

    python tools/bench_match_large_k.py --out DIR [--quick] [--ks 1,16,17,100,1000,G] [--tag SUFFIX]

Writes one JSON line per configuration to stdout and DIR/match_large_k{SUFFIX}.jsonl, and a markdown table to
DIR/match_large_k{SUFFIX}.md.
`--quick` (one window of a few calls per configuration) is the form to run under a kernel tracer."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(200, 10000, 512), (1600, 10000, 1024)]
DTYPES = [torch.bfloat16, torch.float32]


def _time(fn, windows, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1000.0 / calls)
    return statistics.median(per_call), min(per_call), max(per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True, help='directory of the result files')
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--ks', default='1,16,17,100,1000,G', help='comma-separated k values; G = the gallery size')
    ap.add_argument('--tag', default='', help='suffix of the output files')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_match_large_k: no GPU')
    from cvpce_amd import ops
    from cvpce_amd._lib import lib
    T = torch.ops.cvpce_amd
    dev = torch.device('cuda:0')
    windows, calls = (1, 3) if args.quick else (7, 20)
    os.makedirs(args.out, exist_ok=True)
    rows = []
    for qn, gn, d in SHAPES:
        g = torch.Generator().manual_seed(qn + gn + d)
        G32 = F.normalize(torch.rand(gn, d, generator=g), dim=1)
        Q32 = F.normalize(torch.rand(qn, d, generator=g), dim=1)
        for dtype in DTYPES:
            Q, G = Q32.to(dtype).to(dev), G32.to(dtype).to(dev)
            qnorm, gnorm = ops.row_norms(Q), ops.row_norms(G)
            for k in [gn if v == 'G' else int(v) for v in args.ks.split(',')]:
                ws = torch.empty(int(lib.cvpce_match_workspace_bytes(qn, gn, k)), dtype=torch.uint8, device=dev)
                idx = torch.empty((qn, k), dtype=torch.int64, device=dev)
                dist = torch.empty((qn, k), dtype=torch.float32, device=dev)
                ours = _time(lambda: T.match_topk(Q, G, qnorm, gnorm, k, ws, idx, dist), windows, calls)
                yard = _time(lambda: torch.topk(torch.mm(Q, G.t()), k, dim=1, largest=True, sorted=True), windows, calls)
                r = {'Q': qn, 'G': gn, 'D': d, 'dtype': str(dtype).replace('torch.', ''), 'k': k, 'us': round(ours[0], 2),
                     'us_min': round(ours[1], 2), 'us_max': round(ours[2], 2), 'torch_mm_topk_us': round(yard[0], 2),
                     'workspace_mb': round(ws.numel() / 2 ** 20, 1), 'windows': windows, 'calls': calls}
                rows.append(r)
                print(json.dumps(r), flush=True)
                del ws, idx, dist
            torch.cuda.empty_cache()
    with open(os.path.join(args.out, f'match_large_k{args.tag}.jsonl'), 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
    with open(os.path.join(args.out, f'match_large_k{args.tag}.md'), 'w') as f:
        f.write('| Q x G x D | dtype | k | cvpce_match_topk us (median; min-max) | torch mm+topk us | workspace MB |\n|---|---|---|---|---|---|\n')
        for r in rows:
            f.write(f"| {r['Q']} x {r['G']} x {r['D']} | {r['dtype']} | {r['k']} | {r['us']} ({r['us_min']}-{r['us_max']}) | "
                    f"{r['torch_mm_topk_us']} | {r['workspace_mb']} |\n")


if __name__ == '__main__':
    main()
