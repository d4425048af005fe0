"""What the 3x3 halo entry points of the C ABI accept and refuse, decided on the host with no device: a refused argument returns 1 and
N <= 0 returns 0 before any HIP call, and an accepted call fails at its first HIP call (code 2) when no GPU is there.  So on a
machine without a GPU the return code tells the whole accept / refuse decision.  Pointers are the dummy 256 or null; nothing reads
them.  tests/test_halo_host_cpu.py replays the cases against the committed table tests/halo_host_cases.json;
`CVPCE_LIB=<library> python tests/halo_host_cases.py --write` rewrites the table from that library (the table in the tree was
written from the library of the commit before csrc/halo_common.h and csrc/worklist.h).  NEVER with a GPU in the machine: an accepted
call would launch on the dummy pointers -- the recorder exits and the test skips there.
(Not a test module.)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TABLE = os.path.join(ROOT, 'tests', 'halo_host_cases.json')

P = 256      # the dummy pointer

# entry point -> its parameters in order ('stream' is always null)
_CONV = ['in', 'wgt', 'bias', 'out', 'N', 'H', 'W', 'Cin', 'Cout', 'K_pad', 'Cout_pad', 'relu', 'pool', 'stream']
_MAC = ['in', 'wgt', 'bias', 'out', 'mac', 'mac_stride', 'mac_off', 'N', 'H', 'W', 'Cin', 'Cout', 'K_pad', 'Cout_pad', 'pool', 'stream']
_MASKED = ['in', 'wgt', 'bias', 'mask', 'tile_map', 'n_map', 'out', 'N', 'H', 'W', 'Cin', 'Cout', 'K_pad', 'Cout_pad', 'relu', 'stream']
_THIN = ['in', 'wgt', 'bias', 'out', 'N', 'H', 'W', 'Cin', 'Cout', 'K_pad', 'Cout_pad', 'stream']
_LIST = ['in', 'wgt', 'bias', 'out', 'mac', 'mac_stride', 'mac_off', 'N', 'H', 'W', 'Cin', 'Cout', 'K_pad', 'Cout_pad', 'relu', 'pool',
         'list', 'count', 'stream']
ENTRIES = {
    'cvpce_conv3x3_halo': _CONV, 'cvpce_conv3x3_halo_f16': _CONV, 'cvpce_conv3x3_halo_mac': _MAC,
    'cvpce_conv3x3_halo_masked': _MASKED, 'cvpce_conv3x3_halo_masked_f16': _MASKED,
    'cvpce_conv3x3_halo_wide': _CONV, 'cvpce_conv3x3_halo_wide_f16': _CONV,
    'cvpce_conv3x3_halo_thin_out': _THIN, 'cvpce_conv3x3_halo_thin_out_f16': _THIN,
    'cvpce_conv3x3_halo_list': _LIST, 'cvpce_conv3x3_halo_strips': _LIST,
}
# the valid call every case is one step away from; K_pad / Cout_pad None: 9 Cin / Cout rounded up to 256.  `mac` is null where it is
# optional (the list entries) and set where the entry is about it
BASE = dict({'in': P, 'wgt': P, 'bias': P, 'out': P, 'mask': P, 'list': P, 'count': P, 'stream': 0}, mac=0, mac_stride=0, mac_off=0,
            tile_map=0, n_map=0, N=2, H=32, W=48, Cin=64, Cout=256, K_pad=None, Cout_pad=None, relu=1, pool=0)
MAC_ON = dict(mac=P, mac_stride=512, mac_off=0)


def variations():
    """(label, overrides): each flips one condition of a dispatcher, on one side of its boundary."""
    v = [('base', {})]
    v += [(f'null {k}', {k: 0}) for k in ('in', 'wgt', 'bias', 'out', 'mask', 'list', 'count')]
    v += [('mac', MAC_ON), ('mac no out', dict(MAC_ON, out=0)), ('no mac no out', dict(out=0, mac=0)), ('mac no relu', dict(MAC_ON, relu=0)),
          ('mac off -1', dict(MAC_ON, mac_off=-1)), ('mac off fits', dict(MAC_ON, mac_off=256)), ('mac off over', dict(MAC_ON, mac_off=257)),
          ('mac cout 128', dict(MAC_ON, Cout=128)), ('mac cout 136', dict(MAC_ON, Cout=136)), ('mac pool', dict(MAC_ON, pool=1))]
    v += [('map', dict(tile_map=P, n_map=4)), ('map n 0', dict(tile_map=P, n_map=0)), ('map n -1', dict(tile_map=P, n_map=-1)),
          ('map no mask', dict(tile_map=P, n_map=4, mask=0)), ('map cout 128', dict(tile_map=P, n_map=4, Cout=128)),
          ('map too many tiles', dict(tile_map=P, n_map=1 << 29))]
    v += [(f'N {n}', dict(N=n)) for n in (0, -1, 1)]
    v += [(f'Cin {c}', dict(Cin=c)) for c in (128, 96, 32, 0, -64)]
    v += [(f'Cout {c}', dict(Cout=c)) for c in (0, -8, 8, 9, 12, 36, 120, 124, 128, 129, 132, 136, 260, 264, 512)]
    v += [(f'H {h}', dict(H=h)) for h in (0, -2, 1, 13)] + [(f'W {w}', dict(W=w)) for w in (0, -2, 1, 13)]
    v += [('pool', dict(pool=1)), ('pool odd H', dict(pool=1, H=31)), ('pool odd W', dict(pool=1, W=47)), ('odd H', dict(H=31)), ('odd W', dict(W=47)),
          ('pool cout 128', dict(pool=1, Cout=128)), ('pool odd H cout 128', dict(pool=1, H=31, Cout=128))]
    v += [('K_pad +1', dict(K_pad=577)), ('K_pad -1', dict(K_pad=575)), ('K_pad 0', dict(K_pad=0)),
          ('Cout_pad +128', dict(Cout_pad=384)), ('Cout_pad +256', dict(Cout_pad=512)), ('Cout_pad 0', dict(Cout_pad=0)),
          ('Cout_pad below Cout', dict(Cout=264, Cout_pad=256)), ('Cout_pad 32', dict(Cout=8, Cout_pad=32))]
    # N H W Cin 2 < 2^32 bytes of input; N H W Cout < 2^31 output elements; Cout_pad K_pad 2 < 2^31 bytes of weights
    for cout in (256, 128, 9):
        v += [(f'in bytes under cout {cout}', dict(N=4, H=1024, W=1023, Cin=512, Cout=cout)), (f'in bytes at cout {cout}', dict(N=4, H=1024, W=1024, Cin=512, Cout=cout))]
    v += [('out elems under', dict(N=8, H=1024, W=1023)), ('out elems at', dict(N=8, H=1024, W=1024)),
          ('out elems under cout 128', dict(N=16, H=1024, W=1023, Cout=128)), ('out elems at cout 128', dict(N=16, H=1024, W=1024, Cout=128))]
    for cout in (256, 128):
        v += [(f'wgt bytes under cout {cout}', dict(Cout=cout, Cout_pad=1863936)), (f'wgt bytes at cout {cout}', dict(Cout=cout, Cout_pad=1864192))]
    # tile-chunks of a launch: below 2^30 (16-wide tiles, 256-cout tiles), below 2^29 (32-wide tiles, 128-cout tiles); one-pixel images
    big = dict(H=1, W=1, Cin=10816, Cout=10816, Cout_pad=11008)          # 43 cout tiles x 169 chunks = 7267 per image
    n30 = -(-(1 << 30) // 7267)
    v += [('chunks 2^30 under', dict(big, N=n30 - 1)), ('chunks 2^30 at', dict(big, N=n30))]
    wide = dict(H=1, W=1, Cin=8192, Cout=8192, Cout_pad=8192)            # 64 cout tiles x 128 chunks = 2^13 per image
    v += [('chunks 2^29 under', dict(wide, N=(1 << 16) - 1)), ('chunks 2^29 at', dict(wide, N=1 << 16))]
    # what a work-list entry can hold (csrc/worklist.h): images, tile rows / columns of both tile widths, extents
    for cout in (256, 128):
        c = f' cout {cout}'
        v += [('N 65535' + c, dict(N=65535, H=8, W=8, Cout=cout)), ('N 65536' + c, dict(N=65536, H=8, W=8, Cout=cout)),
              ('N 65535 pool' + c, dict(N=65535, H=8, W=8, Cout=cout, pool=1))]
        v += [(f'H {h}' + c, dict(N=1, H=h, W=16, Cout=cout)) for h in (4080, 4081, 4095, 4096)]
        v += [(f'W {w}' + c, dict(N=1, H=16, W=w, Cout=cout)) for w in (4080, 4081, 4095, 4096, 8160, 8161)]
    v += [('mac H 4080', dict(MAC_ON, N=1, H=4080, W=16)), ('mac W 4081', dict(MAC_ON, N=1, H=16, W=4081))]
    return v


def cases():
    """{name: (entry point, argument tuple)}; a variation that names a parameter an entry point does not have is left out there."""
    out = {}
    for fn, params in ENTRIES.items():
        seen = set()
        for label, over in variations():
            if not set(over) <= set(params):
                continue
            a = dict(BASE, **over)
            if fn == 'cvpce_conv3x3_halo_mac' and 'mac' not in over:
                a.update(MAC_ON)
            if fn.startswith('cvpce_conv3x3_halo_thin_out') and 'Cout' not in over:
                a['Cout'] = 36
            if a['K_pad'] is None:
                a['K_pad'] = 9 * a['Cin']
            if a['Cout_pad'] is None:
                a['Cout_pad'] = (a['Cout'] + 255) // 256 * 256
            args = tuple(a[p] for p in params)
            if args in seen:
                continue
            seen.add(args)
            out[f'{fn[len("cvpce_conv3x3_"):]}: {label}'] = (fn, args)
    return out


def gpu_visible():
    import torch
    return os.path.exists('/dev/kfd') or torch.cuda.is_available()


def run(lib):
    """{name: return code} of every case on `lib` (cvpce_amd._lib.lib).  The caller has made sure that no GPU is visible."""
    return {name: int(getattr(lib, fn)(*args)) for name, (fn, args) in cases().items()}


if __name__ == '__main__':
    if sys.argv[1:] != ['--write']:
        sys.exit('usage: CVPCE_LIB=<library> python tests/halo_host_cases.py --write')
    if gpu_visible():
        sys.exit('a GPU is visible: an accepted case would launch a kernel on dummy pointers')
    from cvpce_amd._lib import lib, LIB_PATH
    codes = run(lib)
    with open(TABLE, 'w') as f:
        json.dump(codes, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{len(codes)} cases from {LIB_PATH}: ' + ', '.join(f'{list(codes.values()).count(c)} x {c}' for c in (0, 1, 2)))
