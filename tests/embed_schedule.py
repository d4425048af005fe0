"""The embedder's schedule launch by launch, worked out on the host: `MACVGGEngine.embed_packed` runs on CPU tensors (allocated, never
read) inside `conv_routes.stubbed`, with a recorder in place of the custom-op namespace that notes WHICH tensor every op got: a tensor
argument is [shape, storage offset], so row k + j of the packed work lists is told from row j and a one-element slice of the counts
from its neighbours.  With a ConvProfile set, the records filed (they feed bench.py's `flops_executed`) are noted the same way.
tests/test_embed_schedule_cpu.py replays the cases against the committed table tests/embed_schedule.json;
`python tests/embed_schedule.py --write` rewrites the table from the tree it runs in.  The table was written from the code that
preceded the typed schedule (`SkipSchedule`, `SkipLayer`, `WorkLists`); it changes only with a change that means to change a launch.
Uses only `embed_packed`, `const_crop`, `skip_plan`'s three-way result, the module switches and VGG_CFGS.
(Not a test module.)"""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import conv_routes  # noqa: E402

TABLE = os.path.join(ROOT, 'tests', 'embed_schedule.json')
S = 256
BATCH_LIMITS = dict(FUSED_EMBED_BATCH=8, FUSED_EMBED_MAX=12, LATE_EMBED_MAX=30)      # 37 crops: two late passes (30 + 7 crops), five early ones (8 + 8 + 8 + 6, 7)
TAIL = (512, 512, 512, 'M', 512, 512, 512, 'M')
EXTRA_CFGS = {'wide after 16x16': (64, 64, 'M', 256, 128, 'M', 256, 256, 256, 'M') + TAIL,     # a wide-tile layer after a 16 x 16-tile one: everything in passes
              'early 1': (64, 64, 'M', 256, 256, 'M', 256, 256, 256, 'M') + TAIL}              # the first conv after the stem is a late layer: `big[...].copy_`


def _case(name, model='vgg16', n=37, channels=4, calls=1, want_bf16=False, partial=False, **switches):
    return dict(name=name, model=model, n=n, channels=channels, calls=calls, want_bf16=want_bf16, partial=partial, switches=switches)


DEFAULT = 'default, N = 37'
CASES = [
    _case(DEFAULT),
    _case('default, N = 37, want_bf16', want_bf16=True),
    _case('default, N = 1', n=1),
    _case('default, N = 5', n=5),
    _case('default, N = 0', n=0),
    _case('default, N = 5, want_bf16', n=5, want_bf16=True),
    _case('vgg16_bn', model='vgg16_bn'),
    _case('SKIP_ROWS off', SKIP_ROWS=False),
    _case('SKIP_MAC off', SKIP_MAC=False),
    _case('SKIP_STRIPS off', SKIP_STRIPS=False),
    _case('SKIP_FINE off', SKIP_FINE=False),
    _case('SKIP_FINE_PARTS ()', SKIP_FINE_PARTS=()),
    _case("SKIP_FINE_PARTS ('halo2',)", SKIP_FINE_PARTS=('halo2',)),
    _case("SKIP_FINE_PARTS ('halo3',)", SKIP_FINE_PARTS=('halo3',)),
    _case("SKIP_FINE_PARTS ('halo3', 'halo2', 'thin')", SKIP_FINE_PARTS=('halo3', 'halo2', 'thin')),
    _case('SKIP_PADDING off', SKIP_PADDING=False),
    _case('ops.USE_FUSED_MAC off', USE_FUSED_MAC=False),
    _case('USE_FUSED_STEM off, 8 channels, N = 5', n=5, channels=8, USE_FUSED_STEM=False),
    _case('partial', partial=True),
    _case('cfg: wide after 16x16', model='wide after 16x16'),
    _case('cfg: early 1', model='early 1'),
    _case('second call on the same engine', calls=2),
]
OPS_SWITCHES = ('USE_FUSED_MAC',)      # the switches that live in cvpce_amd.ops; the others in models.classification


def _tensor(t):
    return [list(t.shape), t.storage_offset()]


def _arg(a):
    """-> (True, how a tensor argument is noted) | (False, the scalar)"""
    if a is None:
        return True, None
    if torch.is_tensor(a):
        return True, _tensor(a)
    if isinstance(a, (list, tuple)) and a and all(torch.is_tensor(e) for e in a):
        return True, len(a)
    return False, a


class ArgRecorder:
    """Stands in for `torch.ops.cvpce_amd`: every op called is noted as [name, [per tensor parameter: None | [shape, storage offset] |
    the length of a list of tensors], [the other arguments]]."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(*args):
            noted = [_arg(a) for a in args]
            self.calls.append([name, [v for is_t, v in noted if is_t], [v for is_t, v in noted if not is_t]])
        return op


_MODELS = {}


def _model(name):
    """The models by name, made once (the trace depends on their shapes only)."""
    from cvpce_amd import synthetic
    from cvpce_amd.models import classification as C
    if name not in _MODELS:
        if name in EXTRA_CFGS:
            C.VGG_CFGS[name] = EXTRA_CFGS[name]
            try:
                _MODELS[name] = C.MACVGG(name, batch_norm=False)
            finally:
                del C.VGG_CFGS[name]
        else:
            _MODELS[name] = synthetic.synthetic_macvgg(seed=1, batch_norm=name == 'vgg16_bn')
    return _MODELS[name]


@contextlib.contextmanager
def switched(ops, C, switches):
    todo = [(C, k, v) for k, v in BATCH_LIMITS.items()] + [(ops if k in OPS_SWITCHES else C, k, v) for k, v in switches.items()]
    saved = [(mod, k, getattr(mod, k)) for mod, k, _ in todo]
    for mod, k, v in todo:
        setattr(mod, k, v)
    try:
        yield
    finally:
        for mod, k, v in saved:
            setattr(mod, k, v)


def _plain(v):
    return json.loads(json.dumps(v))


def run_case(case, profile):
    """One case on a fresh engine -> {'calls': the op calls of the last `embed_packed`, 'plan': `skip_plan(S)` as plain lists | None,
    'modes': the layer modes of every distinct `embed_worklists` call [, 'records': what was filed with the profile]}."""
    from cvpce_amd import ops
    from cvpce_amd.models import classification as C
    with switched(ops, C, case['switches']), conv_routes.stubbed(ops):
        rec = ops.T = ArgRecorder()
        eng = C.MACVGGEngine(_model(case['model']), torch.device('cpu'))
        x = torch.empty((case['n'], S, S, case['channels']), dtype=torch.bfloat16)        # never read: its pages are never touched
        ext = torch.zeros((case['n'], 2), dtype=torch.int32)
        const = eng.const_crop(C.TANH_MEAN, C.TANH_STD, case['channels'], S)
        for _ in range(case['calls']):
            del rec.calls[:]
            ops.PROFILE = prof = ops.ConvProfile() if profile else None
            eng.embed_packed(x, want_bf16=case['want_bf16'], ext=ext, const_in=const, partial=case['partial'])
            ops.PROFILE = None
        got = {'calls': list(rec.calls)}
        plan = eng.skip_plan(S)
        if plan is not None:
            steps, layers, pool_mask = plan
            plan = {'layers': [list(l) for l in layers], 'pool_mask': pool_mask,
                    'steps': [[st[0], None if st[1] is None else st[1].cout] + list(st[2:4] if st[0] == 'stem' else st[2:5]) for st in steps]}
        got['plan'] = plan
        modes = []
        for name, _, scalars in rec.calls:
            if name == 'embed_worklists':
                flat = [s for s in scalars if isinstance(s, list)][0]
                if flat[8::9] not in modes:
                    modes.append(flat[8::9])
        got['modes'] = modes
        if profile:
            got['records'] = [[r[0], r[1]] + [_arg(v)[1] for v in r[4:]] for r in prof.records]
    return _plain(got)


def replay(profile=True):
    """-> {case name: what `run_case` gives}, in case order."""
    return {case['name']: run_case(case, profile) for case in CASES}


# The committed form: every distinct call / record is one line of `lines`, and a case lists line numbers.
def pack(table):
    lines, index = [], {}

    def ref(entry):
        key = json.dumps(entry, separators=(',', ':'))
        if key not in index:
            index[key] = len(lines)
            lines.append(key)
        return index[key]

    cases = {name: dict(got, calls=[ref(c) for c in got['calls']], records=[ref(r) for r in got['records']]) for name, got in table.items()}
    return lines, cases


def write_table(table):
    lines, cases = pack(table)
    with open(TABLE, 'w') as f:
        f.write('{"lines": [\n' + ',\n'.join(lines) + '\n],\n"cases": {\n'
                + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in cases.items()) + '\n}}\n')


def load_table():
    with open(TABLE) as f:
        packed = json.load(f)
    lines = packed['lines']
    return {name: dict(got, calls=[lines[i] for i in got['calls']], records=[lines[i] for i in got['records']]) for name, got in packed['cases'].items()}


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/embed_schedule.py --write')
    table = replay()
    write_table(table)
    print(f'{len(table)} cases, {sum(len(g["calls"]) for g in table.values())} op calls, {len(pack(table)[0])} distinct lines -> {TABLE}')
