"""Dev-only: writes tests/golden/gaussian_targets.pt, the vectors that pin the Gaussian-map scoring rule, by running the
reference's own `generate_gaussians` (cvpce/datautils.py:65-85) and `gaussian_loss` (cvpce/models/proposals.py:141-160) under
make_golden.py's import stand-ins.  Data only: the inputs of tests/gaussian_cases.py and what the reference made of them.

    python tests/golden/make_gaussian_golden.py [path of the reference checkout]
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gaussian_cases as gc      # noqa: E402
import make_golden               # noqa: E402


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else make_golden.REF
    make_golden._stub_modules()
    sys.path.insert(0, ref)
    from cvpce import datautils as rd
    from cvpce.models import proposals as rp
    generate = {'multivariate_normal': rd.generate_via_multivariate_normal, 'kant_method': rd.generate_via_kant_method,
                'simple_and_scaled': rd.generate_via_simple_and_scaled}
    joins = {'max': rd.join_via_max, 'addition': rd.join_via_addition, 'replacement': rd.join_via_replacement}

    def run(c):
        return rd.generate_gaussians(c['w'], c['h'], torch.tensor(c['boxes'], dtype=torch.long), size_reduction=c['size_reduction'],
                                     generate_method=generate[c['method']](), join_method=joins[c['join']], tanh=c['tanh'])

    out = {'targets': {}, 'losses': {}}
    for name, c in gc.target_cases():
        out['targets'][name] = dict(c, expected=run(c).clone())
    maps = [run(dict(im, size_reduction=1, method='multivariate_normal', join='max', tanh=False)) for im in gc.LOSS_IMAGES]
    sizes = [im['size'] for im in gc.LOSS_IMAGES]
    # (the maps and the two predictions are stored once; 'no_positives' scores all-zero maps of the same shapes)
    out['losses'] = {'maps': [m.clone() for m in maps], 'sizes': sizes, 'cases': {},
                     'predictions': {'base': torch.from_numpy(gc.loss_predictions('defaults')), 'ties': torch.from_numpy(gc.loss_predictions('ties_at_tau'))}}
    for name, params in gc.LOSS_PARAMS.items():
        which = 'ties' if name == 'ties_at_tau' else 'base'
        targets = [torch.zeros_like(m) for m in maps] if name == 'no_positives' else maps
        out['losses']['cases'][name] = {'prediction': which, 'zero_maps': name == 'no_positives', 'params': dict(params),
                                        'expected': rp.gaussian_loss(out['losses']['predictions'][which], targets, sizes, **params).clone()}
    path = os.path.join(HERE, 'gaussian_targets.pt')
    torch.save(out, path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
