"""Footprint checking for kernel tests: does a kernel read and write only the tensors it is given?  (Not a test module:
test_footprint_cpu.py shows on the host that `check` fails when it should, test_gpu_footprint.py applies it to the HIP kernels.)

A parity test looks at the output tensor only.  Three kinds of error pass it:
  * a store past the output (it lands in the allocator's slack or in a neighbouring tensor);
  * a load past an input whose value reaches the result (the allocator usually leaves zeros or a finite earlier tensor there);
  * an output element that is never written (a second torch.empty of the same shape may still hold an earlier, correct result).

`arena` puts a tensor between two guard bands inside one allocation the test owns.  Input guards are filled, in three runs, with
quiet NaN, the largest finite value and its negative -- three because fmax-style code (max-pool, the MAC / global-max epilogues, a
ReLU written as max(x, 0)) drops a NaN and a ReLU hides a huge negative value: across the three, an out-of-tensor value that reaches
an output element changes it in at least one run.  Output arenas are prefilled as a whole, payload included, with a NaN bit pattern
no kernel computes (integers: 0x5A bytes), so "guard unchanged" and "element never written" are both bit tests.

Every guard band is a multiple of 4 KiB, so a view keeps the alignment of its allocation: pointers with a smaller alignment than
a fresh allocation's are deliberately not produced here.
"""
import torch

FILLS = ('nan', 'max', '-max')          # the three input fills
SCRATCH = 'scratch'                     # `written` entry of a workspace: only its guard bands are checked
GUARD_MIN = 64 << 10
PAGE = 4 << 10
TILE_ROWS = 16

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# prefill bit patterns of float outputs: NaNs (exponent all ones, mantissa non-zero) that are not the canonical quiet NaN an
# arithmetic instruction produces (fp16 0x7E00, bf16 0x7FC0, f32 0x7FC00000, f64 0x7FF8...), so a computed NaN is not mistaken for them
_NAN_PREFILL = {torch.float16: 0x7DA5, torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5}
_INT_PREFILL = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


def guard_bytes(shape, dtype):
    """Bytes of one guard band: the larger of 64 KiB and one full tile row of the tensor (16 rows x W x C elements; W x C = the
    last two dimensions, or the last one of a vector), rounded up to 4 KiB."""
    esz = torch.empty(0, dtype=dtype).element_size()
    shape = tuple(int(s) for s in shape)
    row = 1
    for s in shape[-2:]:
        row *= max(s, 1)
    need = max(GUARD_MIN, TILE_ROWS * row * esz)
    return (need + PAGE - 1) // PAGE * PAGE


def _bits(t):
    """the integer view of a tensor's bytes (same shape)"""
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    return t if t.dtype in _INT_VIEW.values() else t.view(_INT_VIEW[t.element_size()])


def prefill_value(dtype):
    """the bit pattern (as an integer of the element's width) that an output arena holds before the kernel runs"""
    esz = torch.empty(0, dtype=dtype).element_size()
    return _NAN_PREFILL[dtype] if dtype.is_floating_point else _INT_PREFILL[esz]


def _fill_region(region, dtype, fill):
    """region: flat uint8 slice of an arena, element-aligned -> filled with `fill` ('nan' | 'max' | '-max' | 'out')"""
    if region.numel() == 0:
        return
    typed = region.view(dtype if dtype != torch.bool else torch.uint8)
    if fill == 'out':
        _bits(typed).fill_(prefill_value(dtype))
    elif not dtype.is_floating_point:
        region.fill_(0x5A)                       # integer inputs: counts, work lists, tile maps, masks
    elif fill == 'nan':
        typed.fill_(float('nan'))
    else:
        big = torch.finfo(dtype).max             # 65504 for fp16, bf16's and f32's own largest finite value
        typed.fill_(big if fill == 'max' else -big)


def _span(view, whole):
    """byte offset and byte length of `view` inside `whole`"""
    off = view.data_ptr() - whole.data_ptr()
    nbytes = view.numel() * view.element_size()
    assert view.is_contiguous() and 0 <= off and off + nbytes <= whole.numel()
    return off, nbytes


def arena(shape, dtype, device, fill):
    """-> (view, whole): `whole` is one flat uint8 allocation, `view` a contiguous window of `shape` / `dtype` inside it with a guard
    band of `guard_bytes` before and after it.  fill 'nan' | 'max' | '-max': an input arena (guards AND payload take the fill; the caller
    copies the data into `view`); fill 'out': an output arena, the whole allocation prefilled with `prefill_value`."""
    assert fill in FILLS + ('out',)
    shape = tuple(int(s) for s in shape)
    esz = torch.empty(0, dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    g = guard_bytes(shape, dtype)
    whole = torch.empty(g + numel * esz + g, dtype=torch.uint8, device=device)
    _fill_region(whole[:g], dtype, fill)
    _fill_region(whole[g:g + numel * esz], dtype, fill)
    _fill_region(whole[g + numel * esz:], dtype, fill)
    view = whole[g:g + numel * esz].view(dtype if dtype != torch.bool else torch.uint8).view(shape)
    if dtype == torch.bool:
        view = view.view(torch.bool)
    return view, whole


def put(t, device, fill='nan'):
    """an input arena holding a copy of `t` (None passes through): -> (view, whole)"""
    if t is None:
        return None
    view, whole = arena(t.shape, t.dtype, device, fill)
    view.copy_(t)
    return view, whole


def out(shape, dtype, device):
    """an output (or workspace) arena: -> (view, whole)"""
    return arena(shape, dtype, device, 'out')


def _refill_guards(pair, fill):
    view, whole = pair
    off, nbytes = _span(view, whole)
    _fill_region(whole[:off], view.dtype, fill)
    _fill_region(whole[off + nbytes:], view.dtype, fill)


def _sync(pairs):
    if any(whole.is_cuda for _, whole in pairs):
        torch.cuda.synchronize()


def check(run, inputs, outputs, written=None, fills=FILLS):
    """Runs `run()` once per fill and asserts, bit for bit:
      1. every output guard band still holds its prefill;
      2. every input arena, guards and payload, is unchanged (a kernel does not write its inputs);
      3. every element of every output view was written -- no prefill pattern is left.  `written`: where the contract says only a part
         is written, a boolean mask broadcastable to the view (one output) or a list with one entry per output: elements outside
         the mask must still hold the prefill, elements inside it must not.  An entry may also be None (everything is written), a pair
         (must, may) of masks where the contract leaves some elements open (those in `must` are written, those outside `may` are
         not), or SCRATCH (a workspace: no claim about its contents, only its guard bands are checked);
      4. the written elements of the output views are bit-identical across the runs, and finite where they are floats.  Finiteness
         goes by the arena's own element type: a block of mixed fields held as integers (the int32 block of detect_postprocess, with
         f32 boxes and scores inside it) gets the bit comparison only, and its caller checks the float fields against its reference.
    inputs / outputs: lists of (view, whole) pairs of `arena` (None entries are skipped).  Before each run the input guards take that
    run's fill and the output arenas their prefill.  -> clones of the output views after the last run, in the order of `outputs`."""
    inputs = [p for p in inputs if p is not None]
    outputs = [p for p in outputs if p is not None]
    if written is None or torch.is_tensor(written) or isinstance(written, (tuple, str)):
        written = [written] + [None] * (len(outputs) - 1)
    assert len(written) == len(outputs)
    masks = []          # per output: None | SCRATCH | (must, may)
    for (view, _), m in zip(outputs, written):
        if m is not None and m is not SCRATCH:
            must, may = m if isinstance(m, tuple) else (m, m)
            m = tuple(torch.as_tensor(t, dtype=torch.bool).to(view.device).expand(view.shape) for t in (must, may))
            assert not bool((m[0] & ~m[1]).any())
        masks.append(m)
    results = []
    for fill in fills:
        for pair in inputs:
            _refill_guards(pair, fill)
        before = [whole.clone() for _, whole in inputs]
        for view, whole in outputs:
            _fill_region(whole, view.dtype, 'out')
        _sync(inputs + outputs)
        run()
        _sync(inputs + outputs)
        for i, (view, whole) in enumerate(outputs):                                               # 1
            off, nbytes = _span(view, whole)
            pre = prefill_value(view.dtype)
            for name, band in (('before', whole[:off]), ('after', whole[off + nbytes:])):
                b = _bits(band.view(view.dtype if view.dtype != torch.bool else torch.uint8))
                assert torch.equal(b, torch.full_like(b, pre)), \
                    f'fill {fill}: output {i}: the guard band {name} the tensor was written ({int((b != pre).sum())} elements changed, ' \
                    f'first at guard element {int((b != pre).nonzero()[0])} of {b.numel()})'
        for i, ((view, whole), snap) in enumerate(zip(inputs, before)):                           # 2
            assert torch.equal(whole, snap), f'fill {fill}: input {i} (or its guard bands) was written'
        for i, ((view, whole), m) in enumerate(zip(outputs, masks)):                              # 3
            if m is SCRATCH:
                continue
            stale = _bits(view) == prefill_value(view.dtype)
            if m is None:
                assert not bool(stale.any()), \
                    f'fill {fill}: output {i}: {int(stale.sum())} elements never written, first at {stale.nonzero()[0].tolist()}'
            else:
                bad = stale & m[0]
                assert not bool(bad.any()), \
                    f'fill {fill}: output {i}: {int(bad.sum())} elements the contract writes were not written, first at {bad.nonzero()[0].tolist()}'
                bad = ~stale & ~m[1]
                assert not bool(bad.any()), \
                    f'fill {fill}: output {i}: {int(bad.sum())} elements outside the written part changed, first at {bad.nonzero()[0].tolist()}'
        results.append([view.clone() for view, _ in outputs])
    for i, ((view, _), m) in enumerate(zip(outputs, masks)):                                      # 4
        if m is SCRATCH:
            continue
        sel = (lambda t: t) if m is None else (lambda t, m=m: t[m[0]])
        first = sel(_bits(results[0][i]))
        for fill, res in zip(fills[1:], results[1:]):
            same = sel(_bits(res[i])) == first
            assert bool(same.all()), \
                f'output {i} differs between the fills {fills[0]} and {fill} in {int((~same).sum())} elements: a value from outside an input reached it'
        if view.dtype.is_floating_point:
            for fill, res in zip(fills, results):
                assert bool(torch.isfinite(sel(res[i])).all()), f'fill {fill}: output {i} holds non-finite values'
    return results[-1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the embedder's work lists (test_gpu_footprint.py test_list_and_strip_launches, test_gpu_exact.py): which pixels a list covers, the
# lists themselves in plain Python, and a layer's input as the lists left it
# ---------------------------------------------------------------------------------------------------------------------------------
def listed_pixels(entries, n, h, w, th, tw):
    """(n,h,w,1) bool: the output pixels the tiles of a work list cover -- entry = (rows << 56 | ...) | n << 16 | ty << 8 | tx
    (include/cvpce_amd.h): a tile cut at `rows` of its 16 conv-output rows stores that share of its th output rows."""
    m = torch.zeros(n, h, w, 1, dtype=torch.bool)
    for e in entries:
        rows, img, ty, tx = (e >> 56) & 0xFF, (e >> 16) & 0xFFFF, (e >> 8) & 0xFF, e & 0xFF
        m[img, ty * th:ty * th + rows * th // 16, tx * tw:(tx + 1) * tw] = True
    return m


def worklist_model(ext, size, pool_mask, layers):
    """The work lists of include/cvpce_amd.h (cvpce_embed_worklists) in plain Python, independent of the kernel -- the model of
    tests/test_gpu_skip.py test_worklists_match_python_model at crop size `size`.  ext: (rows, cols) per crop, the constant crop
    included -> per layer (list entries, strip-list entries, MFMA work in sixteenths of a tile, [rows computed, tile columns] per crop)."""
    def extent(e0, nops, dim):
        if e0 >= size:
            return dim
        e = e0
        for i in range(nops):
            e = (e + 1) // 2 if (pool_mask >> i) & 1 else e + 1
        return min(dim, e)
    model = []
    for h, w, th, tw, out_ops, ih, iw, in_ops, skip in layers:
        ty_n, tx_n = -(-h // th), -(-w // tw)
        want, swant, comp = [], [], []
        for c, (ey0, ex0) in enumerate(ext):
            ny, nx = ty_n, tx_n
            if skip:
                ny = min(ty_n, -(-extent(ey0, out_ops, h) // th))
                nx = min(tx_n, -(-extent(ex0, out_ops, w) // tw))
            if nx == 0:
                ny = 0                                           # no tile column listed: no tile row either
            ext_in = (extent(ey0, in_ops, ih) << 12) | extent(ex0, in_ops, iw)
            last = 16
            for ty in range(ny):
                rows = 16
                if skip >= 2 and ty == ny - 1:
                    act = min(th, extent(ey0, out_ops, h) - ty * th)
                    last = rows = min(16, (-(-act * 16 // th) + 3) // 4 * 4)
                entries = [(((rows << 24) | ext_in) << 32) | (c << 16) | (ty << 8) | tx for tx in range(nx)]
                if skip >= 3 and rows == 4 and ty == ny - 1:
                    swant += entries
                else:
                    want += entries
            comp.append([(ny - 1) * 16 + last if ny else 0, nx])
        work = sum(r + 1 if r < 16 else 16 for r in ((e >> 56) & 0xFF for e in want)) + 4 * len(swant)
        model.append((want, swant, work, comp))
    return model


def whole(prev, mask):
    """the tensor a layer's list leaves to the constant crop, filled in from the constant crop's own pixels (image n - 1)"""
    prev = prev.cpu()
    return torch.where(mask.expand_as(prev), prev, prev[-1:].expand_as(prev))
