"""Dev-only: writes tests/golden/tonioni.pt, the vectors that pin the Tonioni matcher (the Tonioni rule), by running the
reference's own `build_graph`, `tonioni_mcs` and `large_common_subgraph` (cvpce/planograms.py:30-169) under make_golden.py's import
stand-ins.  Data only: the inputs of tests/tonioni_cases.py and what the reference made of them.

    python tests/golden/make_tonioni_golden.py [path of the reference checkout]
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import tonioni_cases as tc       # noqa: E402
import make_golden               # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    make_golden._stub_modules()
    sys.modules['cv2'].findHomography, sys.modules['cv2'].RANSAC = None, 8      # (imported by name, never called here)
    sys.path.insert(0, ref)
    from cvpce import planograms as rp
    out = []
    for c in tc.cases():
        g1, g2 = rp.build_graph(c['boxes1'], c['labels1']), rp.build_graph(c['boxes2'], c['labels2'])
        found = rp.tonioni_mcs(g1, g2, min_score=c['min_score'])
        large = rp.large_common_subgraph(g1, g2, min_score=c['min_score'])
        out.append(dict(c, tonioni=sorted((int(a), int(b)) for a, b in found), large=len(large),
                        hypotheses=len(rp.build_hypotheses(g1, g2))))
        print(c['name'], out[-1]['hypotheses'], len(found), len(large))
    path = os.path.join(HERE, 'tonioni.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
