"""Which launch `ops.conv2d` and the other profiled wrappers of cvpce_amd/ops.py make, and what they file with a ConvProfile, worked
out on the host: the custom-op namespace `ops.T` is replaced by a recorder, so the wrappers run on CPU tensors (allocated, never
read) and no device is touched.  tests/test_conv_routes_cpu.py replays the cases against the committed table
tests/conv_routes.json; `python tests/conv_routes.py --write` rewrites the table from the ops.py of the tree it runs in.  The table
lists a case of the second storage type or of a flipped switch only where it differs from the same case in bf16 or with no switch
flipped (`like`, `shorten`);
the test compares every case all the same.
(Not a test module.)"""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'conv_routes.json')

# (cin, cout, k, stride, pad): the detector's and the embedder's layer shapes
LAYERS = [(64, 64, 1, 1, 0), (64, 256, 1, 1, 0), (256, 64, 1, 1, 0), (64, 64, 3, 1, 1), (256, 512, 1, 2, 0), (512, 128, 1, 1, 0),
          (128, 128, 3, 2, 1), (512, 512, 3, 1, 1), (2048, 256, 1, 1, 0), (256, 256, 3, 1, 1), (256, 256, 3, 2, 1), (256, 9, 3, 1, 1),
          (256, 36, 3, 1, 1), (64, 32, 3, 1, 1), (32, 32, 3, 1, 1), (32, 16, 3, 1, 1), (16, 16, 1, 1, 0), (16, 1, 1, 1, 0),
          (3, 64, 7, 2, 3), (64, 128, 3, 1, 1), (128, 128, 3, 1, 1), (128, 256, 3, 1, 1)]
MAPS = [(1, 16, 16), (2, 25, 25), (1, 50, 52), (1, 100, 100), (4, 200, 200)]     # (n, h, w)
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
# every switch the GPU tests flip, with its other value(s)
SWITCHES = [('USE_HALO_3X3', False), ('USE_CONV1X1', False), ('USE_THIN_3X3', False), ('USE_HALO_THIN_OUT', False), ('CONV_SPLITK', False),
            ('HALO_RAGGED', True), ('CONV1X1_ANY_SHAPE', True), ('FORCE_GENERIC_CONV', True)]

OPS_CONV2D = {'conv2d_nhwc', 'conv2d_splitk', 'conv1x1_nhwc', 'conv3x3_halo', 'conv3x3_halo_thin_out', 'conv3x3_thin'}
RECORD_NAMES_CONV2D = {'conv_igemm_kernel<128,128,64,2,2>', 'conv_igemm_kernel<64,128,32,2,2>', 'conv_igemm_kernel<64,128,64,2,2>',
                       'conv_igemm_kernel<32,128,64,1,4>', 'conv_dma16_kernel<256,256,2,4,2,4>', 'conv_dma_kernel<128,128,2,2,2>',
                       'conv_dma_kernel<64,128,2,2,2>', 'conv1x1_kernel', 'conv3x3_halo2_kernel', 'conv3x3_halo3_kernel', 'thin3x3_kernel'}


class Recorder:
    """Stands in for `torch.ops.cvpce_amd`: every op called is noted as [name, which tensor arguments it got, the other arguments].
    The second entry has one letter per tensor parameter: 't' a tensor, 'n' None, 'l' a list of tensors (its length follows)."""

    def __init__(self):
        self.calls, self.at = [], []       # at: how many events had been recorded when the op was called

    def __getattr__(self, name):
        def op(*args):
            tensors, scalars = '', []
            for a in args:
                if a is None or torch.is_tensor(a):
                    tensors += 'n' if a is None else 't'
                elif isinstance(a, (list, tuple)) and a and all(torch.is_tensor(e) for e in a):
                    tensors += f'l{len(a)}'
                else:
                    scalars.append(a)
            self.calls.append([name, tensors] + scalars)
            self.at.append(Event.recorded)
        return op


class Event:
    """Stands in for torch.cuda.Event; counts how many are made, and numbers them as they are recorded."""
    made = recorded = 0

    def __init__(self, enable_timing=False):
        Event.made += 1

    def record(self):
        Event.recorded += 1
        self.at = Event.recorded

    def elapsed_time(self, other):
        return 0.0


@contextlib.contextmanager
def stubbed(ops):
    """`ops` with the recorder as T, no CPU-tensor refusal and dummy events; everything is put back on exit."""
    saved = ops.T, ops._need_cuda, torch.cuda.Event, ops.PROFILE
    rec = ops.T = Recorder()
    ops._need_cuda = lambda *ts: None
    torch.cuda.Event = Event
    Event.made = 0
    try:
        yield rec
    finally:
        ops.T, ops._need_cuda, torch.cuda.Event, ops.PROFILE = saved


def _scalar(v):
    return v.item() if torch.is_tensor(v) else v


def run(ops, rec, call, profile):
    """One case: -> [the op calls made] (+ with profile: the records, layer records and byte records it filed, without the events --
    of them only this is checked: each pair was recorded around exactly one op call)."""
    del rec.calls[:], rec.at[:]
    ops.PROFILE = prof = ops.ConvProfile() if profile else None
    call()
    got = [list(rec.calls)]
    if profile:
        for r in list(prof.records) + [r[1:] for r in prof.layer_records] + prof.byte_records:
            assert sum(r[2].at <= at < r[3].at for at in rec.at) == 1, (r, rec.calls)
        got += [[list(r[:2]) + [_scalar(v) for v in r[4:]] for r in prof.records],
                [list(r[:3]) for r in prof.layer_records], [list(r[:2]) for r in prof.byte_records]]
    ops.PROFILE = None
    return got


_CACHE = {}


def _conv(ops, cin, cout, k, stride, pad, dtype):
    key = ('conv', cin, cout, k, stride, pad, dtype)
    if key not in _CACHE:
        _CACHE[key] = ops.PackedConv(torch.zeros(cout, cin, k, k), torch.zeros(cout), stride, pad, device='cpu', dtype=dtype)
    return _CACHE[key]


def _empty(shape, dtype):
    key = ('x', tuple(shape), dtype)
    if key not in _CACHE:
        _CACHE[key] = torch.empty(shape, dtype=dtype)      # never read: its pages are never touched
    return _CACHE[key]


def conv2d_cases(ops):
    """-> [(group, key, thunk)]: dtypes x layers x maps x (out_f32 off with ReLU | on without), + a same-size residual for the 1x1s,
    + in_up_shift = 1 for 64 -> 32, + pool for 3x3 / s1 layers with Cout >= 64 on even maps; then the three largest maps again under
    each entry of SWITCHES; then one halo launch filed while the profile's stage is 'detect'."""
    def variants(layer, m):
        cin, cout, k, stride, pad = layer
        v = [dict(out_f32=False), dict(out_f32=True)]
        if k == 1:
            v.append(dict(out_f32=False, res=True))
        if (cin, cout) == (64, 32):
            v.append(dict(out_f32=False, in_up_shift=1))
        if k == 3 and stride == 1 and cout >= 64 and m[1] % 2 == 0 and m[2] % 2 == 0:
            v.append(dict(out_f32=False, pool=True))
        return v

    def thunk(dtype, layer, m, out_f32, res=False, in_up_shift=0, pool=False, switch=None, stage=None):
        def call():
            pc = _conv(ops, *layer, dtype)
            n, h, w = m
            x = _empty((n, h, w, pc.cin_pad), dtype)
            residual = _empty((n,) + pc.out_hw(h, w) + (pc.cout,), dtype) if res else None
            if stage is not None and ops.PROFILE is not None:
                ops.PROFILE.records.stage = stage
            if switch is not None:
                old = getattr(ops, switch[0])
                setattr(ops, switch[0], switch[1])
            try:
                ops.conv2d(x, pc, act=0 if out_f32 else 1, out_f32=out_f32, residual=residual, in_up_shift=in_up_shift, pool=pool)
            finally:
                if switch is not None:
                    setattr(ops, switch[0], old)
        return call

    def key(layer, m, v):
        cin, cout, k, stride, pad = layer
        return (f'{cin}->{cout} k{k} s{stride} p{pad} on {m[0]}x{m[1]}x{m[2]}' + (' f32' if v['out_f32'] else '') + (' +res' if v.get('res') else '')
                + (' up' if v.get('in_up_shift') else '') + (' +pool' if v.get('pool') else ''))

    cases = []
    for switch in [None] + SWITCHES:
        for dn, dtype in DTYPES.items():
            for layer in LAYERS:
                for m in (MAPS if switch is None else MAPS[-3:]):
                    for v in variants(layer, m):
                        group = f'conv2d {dn}' + (f', {switch[0]} = {switch[1]}' if switch else '')
                        cases.append((group, key(layer, m, v), thunk(dtype, layer, m, switch=switch, **v)))
    layer, m = (256, 256, 3, 1, 1), (1, 100, 100)
    cases.append(("conv2d fp16, records.stage = 'detect'", key(layer, m, dict(out_f32=False)), thunk(torch.float16, layer, m, False, stage='detect')))
    return cases


def wrapper_cases(ops):
    """-> [(group, key, thunk)]: the other profiled wrappers, each at the smallest shape its asserts accept."""
    bf, i32 = torch.bfloat16, torch.int32
    z = torch.zeros

    def conv(cin, cout, k, stride=1, pad=0, dtype=bf):
        return _conv(ops, cin, cout, k, stride, pad, dtype)

    def bottleneck():
        x = _empty((1, 16, 16, 256), bf)
        ops.bottleneck(x, conv(256, 64, 1), conv(64, 64, 3, 1, 1), conv(64, 256, 1), x)

    def bottleneck_other_residual():
        ops.bottleneck(_empty((1, 16, 16, 64), bf), conv(64, 64, 1), conv(64, 64, 3, 1, 1), conv(64, 256, 1), _empty((1, 16, 16, 256), bf))

    def relu_mac(**kw):
        return lambda: ops.conv2d_relu_mac(_empty((1, 16, 16, 64), bf), conv(64, 256, 3, 1, 1), z(1, 512), 256, **kw)

    def gln_stem():
        ps = ops.PackedGlnStem(z(64, 3, 7, 7), torch.ones(64), z(64), device='cpu', dtype=torch.float16)
        ops.gln_stem(_empty((1, 16, 16, 8), torch.float16), ps)

    def atlas(**kw):
        return lambda: ops.conv3x3_atlas(_empty((1, 16, 16, 64), bf), conv(64, 256, 3, 1, 1), torch.ones(16, 16, dtype=torch.uint8), **kw)

    def stem():
        return ops.PackedStem(z(64, 3, 3, 3), z(64), z(64, 64, 3, 3), z(64), device='cpu')

    def conv_list(cout, **kw):
        return lambda: ops.conv2d_list(_empty((2, 16, 16, 64), bf), conv(64, cout, 3, 1, 1), z(4, dtype=torch.int64), torch.tensor([3], dtype=i32), **kw)

    def gauss_convs(dtype):
        return [conv(64, 32, 3, 1, 1, dtype), conv(32, 32, 3, 1, 1, dtype), conv(32, 16, 3, 1, 1, dtype), conv(16, 16, 1, dtype=dtype), conv(16, 1, 1, dtype=dtype)]

    def transform(images):
        return lambda: ops.gln_transform_batch(images, _empty((len(images), 16, 16, 8), torch.float16), [(12, 16)] * len(images), (0.4, 0.5, 0.6), (0.2, 0.3, 0.4))

    boxes = torch.tensor([[1., 2., 9., 12.], [0., 0., 16., 16.]])
    ext = torch.tensor([[8, 6], [4, 8]], dtype=i32)

    def crop(img, **kw):
        return lambda: ops.crop_resize(img, boxes, size=8, **kw)

    def u8(thunk):
        def call():
            old, ops.U8_KERNELS = ops.U8_KERNELS, True
            try:
                thunk()
            finally:
                ops.U8_KERNELS = old
        return call

    def postprocess():
        ops.detect_postprocess([z(1, 4 * 4 * 9)], [z(1, 4 * 4 * 9, 4)], [(4, 4)], [(8, 8)], z(9, 4), torch.tensor([[32., 32.]]), torch.ones(1, 2),
                               9, 1, 10, 0.05, 0.5, 4.135, 5, 0.5)

    img_f, img_b = z(3, 16, 16), z(16, 16, 3, dtype=torch.uint8)
    units, strips = torch.tensor([40], dtype=i32), (z(4, dtype=torch.int64), torch.tensor([2], dtype=i32))
    return [('other wrappers',) + c for c in [
        ('bottleneck 256->64->256 on 1x16x16, residual = input', bottleneck),
        ('bottleneck 64->64->256 on 1x16x16', bottleneck_other_residual),
        ('conv2d_relu_mac 64->256 on 1x16x16', relu_mac()),
        ('conv2d_relu_mac 64->256 on 1x16x16 +pool', relu_mac(pool=True)),
        ('conv2d_relu_mac 64->256 on 1x16x16 no store', relu_mac(store=False)),
        ('gln_stem 1x16x16', gln_stem),
        ('conv3x3_atlas 64->256 on 1x16x16', atlas()),
        ('conv3x3_atlas 64->256 on 1x16x16, tile map, 100 mask pixels', atlas(tile_map=z(1, dtype=i32), out=_empty((1, 16, 16, 256), bf), mask_pixels=100)),
        ('vgg_stem 1x16x16x4', lambda: ops.vgg_stem(_empty((1, 16, 16, 4), bf), stem())),
        ('vgg_stem_list 1x16x16x4', lambda: ops.vgg_stem_list(_empty((1, 16, 16, 4), bf), _empty((16, 16, 4), bf), stem(), z(4, dtype=torch.int64), torch.tensor([3], dtype=i32))),
        ('conv2d_list 64->128 on 2x16x16', conv_list(128)),
        ('conv2d_list 64->256 on 2x16x16 +pool, units', conv_list(256, pool=True, units=units)),
        ('conv2d_list 64->256 on 2x16x16 mac, units, strips', conv_list(256, mac=z(2, 512), mac_off=256, units=units, strips=strips)),
        ('conv2d_list 64->256 on 2x16x16 mac, no store, strips', conv_list(256, mac=z(2, 512), store=False, strips=strips)),
        ('gauss_tail 1x8x8x16', lambda: ops.gauss_tail(_empty((1, 8, 8, 16), torch.float16), *gauss_convs(torch.float16)[3:], 2)),
        ('gauss_subnet 1x8x8x64', lambda: ops.gauss_subnet(_empty((1, 8, 8, 64), torch.float16), gauss_convs(torch.float16), 1)),
        ('gln_transform_batch float', transform([img_f])),
        ('gln_transform_batch bytes, U8_KERNELS off', transform([img_b, img_f])),
        ('gln_transform_batch bytes, U8_KERNELS on', u8(transform([img_b, img_f]))),
        ('crop_resize mode 0', crop(img_f)),
        ('crop_resize mode 2', crop(img_f, mode=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))),
        ('crop_resize mode 2, count', crop(img_f, mode=2, count=torch.tensor([1], dtype=i32))),
        ('crop_resize mode 2, content_ext', crop(img_f, mode=2, content_ext=ext)),
        ('crop_resize mode 0 bytes, U8_KERNELS off', crop(img_b)),
        ('crop_resize mode 0 bytes, U8_KERNELS on', u8(crop(img_b))),
        ('crop_resize mode 2 bytes, content_ext, U8_KERNELS on', u8(crop(img_b, mode=2, content_ext=ext))),
        ('detect_postprocess one level', postprocess),
    ]]


def all_cases(ops):
    return conv2d_cases(ops) + wrapper_cases(ops)


def replay(ops, profile=True):
    """-> {group: {key: what `run` gives}}, in case order."""
    table = {}
    with stubbed(ops) as rec:
        for group, key, call in all_cases(ops):
            assert key not in table.setdefault(group, {}), (group, key)
            table[group][key] = run(ops, rec, call, profile)
    return table


BASE = 'conv2d bf16'


def like(group):
    """The group whose results a conv2d group mostly repeats: its bf16 twin for fp16 (the storage type changes no route and no record),
    BASE for a flipped switch; None, or a group that does not exist, for the groups listed in full."""
    if group.startswith('conv2d fp16'):
        return BASE + group[len('conv2d fp16'):]
    return BASE if group.startswith(BASE + ',') else None


def shorten(table):
    """The table as it is committed: a case of a group with a `like` group is listed only where it does NOT give exactly what the case of
    the same key gives there."""
    return {group: {k: v for k, v in cases.items() if like(group) not in table or table[like(group)].get(k) != v} for group, cases in table.items()}


def load_table(ops):
    """The committed table with every case `shorten` left out put back -> {group: {key: expected}} for all of `all_cases`."""
    with open(TABLE) as f:
        short = json.load(f)
    full = {}
    for group, key, _ in all_cases(ops):
        full.setdefault(group, {})[key] = short[group][key] if key in short[group] else full[like(group)][key]
    assert all(set(short[g]) <= set(full.get(g, ())) for g in short), 'the table lists a case that no longer exists'
    return full


def write_table(table):
    """one line per case"""
    table = shorten(table)
    groups = [json.dumps(g) + ': {\n' + ',\n'.join(f'{json.dumps(k)}:{json.dumps(v, separators=(",", ":"))}' for k, v in cases.items()) + '\n}'
              for g, cases in table.items()]
    with open(TABLE, 'w') as f:
        f.write('{\n' + ',\n'.join(groups) + '\n}\n')


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: python tests/conv_routes.py --write')
    from cvpce_amd import ops
    table = replay(ops)
    write_table(table)
    print(f'{sum(len(c) for c in table.values())} cases, {sum(len(c) for c in shorten(table).values())} of them listed -> {TABLE}')
