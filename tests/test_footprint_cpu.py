"""tests/footprint.py fails when it should: small Python "kernels" on CPU arenas, one correct, the others each with one planted
footprint error that `check` must catch with the assertion meant for it.  This is the evidence that a HIP kernel with the same error
would fail tests/test_gpu_footprint.py."""
import pytest
import torch

import footprint as fp            # tests/footprint.py

CPU = torch.device('cpu')
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _flat(pair):
    """(typed flat view of the whole arena, index of the payload's first element, payload elements)"""
    view, whole = pair
    off, nbytes = fp._span(view, whole)
    return whole.view(view.dtype), off // view.element_size(), view.numel()


def _case(dtype, shape=(2, 5, 7, 8)):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(dtype)
    return fp.put(x, CPU), fp.out(shape, dtype, CPU), x


def _raises(match, run, inputs, outputs, **kw):
    with pytest.raises(AssertionError, match=match):
        fp.check(run, inputs, outputs, **kw)


def test_arena_layout():
    for shape, dtype in (((2, 5, 7, 8), torch.bfloat16), ((3, 33, 300, 64), torch.float32), ((5,), torch.int32), ((4, 100), torch.int64)):
        view, whole = fp.arena(shape, dtype, CPU, 'out')
        g = fp.guard_bytes(shape, dtype)
        off, nbytes = fp._span(view, whole)
        assert g % fp.PAGE == 0 and g >= fp.GUARD_MIN and off == g and whole.numel() == 2 * g + nbytes
        assert view.is_contiguous() and tuple(view.shape) == shape and view.dtype == dtype
        assert bool((fp._bits(view) == fp.prefill_value(dtype)).all())
    # one full tile row (16 rows x W x C elements) where that is more than 64 KiB
    assert fp.guard_bytes((3, 33, 300, 64), torch.float32) == 16 * 300 * 64 * 4
    assert fp.guard_bytes((1, 9, 9, 8), torch.bfloat16) == fp.GUARD_MIN
    # the three float fills and the integer fill
    for dtype in DTYPES:
        big = {torch.float16: 65504.0, torch.bfloat16: torch.finfo(torch.bfloat16).max, torch.float32: torch.finfo(torch.float32).max}[dtype]
        assert bool(torch.isnan(fp.arena((3,), dtype, CPU, 'nan')[1].view(dtype)).all())
        assert bool((fp.arena((3,), dtype, CPU, 'max')[1].view(dtype) == big).all())
        assert bool((fp.arena((3,), dtype, CPU, '-max')[1].view(dtype) == -big).all())
        assert bool(torch.isnan(fp.arena((3,), dtype, CPU, 'out')[1].view(dtype)).all())       # the output prefill is a NaN too
    assert bool((fp.arena((3,), torch.int32, CPU, 'nan')[1] == 0x5A).all())
    assert bool((fp.arena((3,), torch.uint8, CPU, 'out')[1] == 0x5A).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_correct_kernel_passes(dtype):
    xin, o, x = _case(dtype)
    got, = fp.check(lambda: o[0].copy_(torch.relu(xin[0])), [xin], [o])
    assert torch.equal(got, torch.relu(x))
    # an integer output next to a float one
    idx = fp.out((2, 5, 7), torch.int64, CPU)

    def run():
        o[0].copy_(xin[0] * 2)
        idx[0].copy_(xin[0].float().argmax(dim=-1))
    got, gi = fp.check(run, [xin], [o, idx])
    assert torch.equal(got, x * 2) and torch.equal(gi, x.float().argmax(dim=-1))


@pytest.mark.parametrize('dtype', DTYPES)
def test_store_past_the_end(dtype):
    xin, o, _ = _case(dtype)
    flat, start, n = _flat(o)

    def run():
        o[0].copy_(xin[0])
        flat[start + n] = 1.0
    _raises('output 0: the guard band after the tensor was written', run, [xin], [o])


@pytest.mark.parametrize('dtype', DTYPES)
def test_store_before_the_start(dtype):
    xin, o, _ = _case(dtype)
    flat, start, n = _flat(o)

    def run():
        o[0].copy_(xin[0])
        flat[start - 1] = 1.0
    _raises('output 0: the guard band before the tensor was written', run, [xin], [o])


@pytest.mark.parametrize('dtype', DTYPES)
def test_element_left_unwritten(dtype):
    xin, o, _ = _case(dtype)

    def run():
        o[0].view(-1)[:-1].copy_(xin[0].view(-1)[:-1])          # the last element of a ragged tile
    _raises(r'output 0: 1 elements never written, first at \[1, 4, 6, 7\]', run, [xin], [o])


def test_unwritten_element_that_still_holds_an_earlier_result():
    """the case a parity test cannot see: the output already holds the right values when the kernel runs -- `check` prefills it"""
    xin, o, x = _case(torch.float32)
    o[0].copy_(x)                                               # what an earlier call of the same shape left behind

    def run():
        o[0][:, :, :6].copy_(xin[0][:, :, :6])                  # column 6 is never stored
    _raises('output 0: 80 elements never written', run, [xin], [o])


@pytest.mark.parametrize('dtype', DTYPES)
def test_store_into_an_input(dtype):
    xin, o, _ = _case(dtype)

    def run():
        o[0].copy_(xin[0])
        xin[0][1, 2, 3, 4] = 0.0
    _raises('input 0 .* was written', run, [xin], [o])
    # and into an input's guard band
    xin, o, _ = _case(dtype)
    flat, start, n = _flat(xin)

    def run():
        o[0].copy_(xin[0])
        flat[start + n + 5] = 0.0
    _raises('input 0 .* was written', run, [xin], [o])


def test_store_into_an_integer_input():
    cnt = fp.put(torch.tensor([3], dtype=torch.int32), CPU)
    o = fp.out((4,), torch.float32, CPU)

    def run():
        o[0].fill_(float(cnt[0][0]))
        cnt[0][0] = 0
    _raises('input 0 .* was written', run, [cnt], [o])


@pytest.mark.parametrize('dtype', DTYPES)
def test_sum_that_includes_a_guard_element(dtype):
    xin, o, _ = _case(dtype, (3, 64))
    so = fp.out((3,), torch.float32, CPU)
    flat, start, n = _flat(xin)

    def run():
        rows = flat[start:start + n + 1].float()                # the last row reads one element too many
        so[0][:2].copy_(rows[:128].view(2, 64).sum(dim=1))
        so[0][2] = rows[128:].sum()
    _raises('output 0 (differs between the fills|holds non-finite)', run, [xin], [so])
    # caught by the NaN fill alone as well: the sum is not finite
    _raises('fill nan: output 0 holds non-finite values', run, [xin], [so], fills=('nan',))


@pytest.mark.parametrize('dtype', DTYPES)
def test_fmax_that_includes_a_guard_element(dtype):
    """fmax drops a NaN: the NaN fill alone cannot see this read, the three fills together do -- the reason for having three"""
    xin, o, x = _case(dtype, (3, 64))
    mo = fp.out((3,), torch.float32, CPU)
    flat, start, n = _flat(xin)

    def run():
        rows = flat[start - 1:start + n].float()                # the first row starts one element early
        rows = torch.fmax(rows, torch.full_like(rows, float('-inf')))   # an fmax accumulator drops a NaN
        mo[0][0] = rows[:65].max()
        mo[0][1:].copy_(rows[65:].view(2, 64).amax(dim=1))
    got, = fp.check(run, [xin], [mo], fills=('nan',))           # passes, and even returns the right answer
    assert torch.equal(got, x.float().amax(dim=1))
    _raises('output 0 differs between the fills nan and max in 1 elements', run, [xin], [mo])


def test_relu_hides_a_negative_guard_value():
    """a max(x, 0) epilogue over one element too many: invisible with NaN (dropped) and with -max (clamped), visible with +max"""
    xin, o, _ = _case(torch.float32, (3, 64))
    mo = fp.out((3,), torch.float32, CPU)
    flat, start, n = _flat(xin)

    def run():
        rows = torch.fmax(flat[start:start + n + 1], torch.zeros(n + 1))
        mo[0][:2].copy_(rows[:128].view(2, 64).amax(dim=1))
        mo[0][2] = rows[128:].max()
    fp.check(run, [xin], [mo], fills=('nan', '-max'))
    _raises('output 0 differs between the fills nan and max', run, [xin], [mo])


def test_partial_write_contract():
    """a list launch: only the listed rows are written"""
    xin, o, x = _case(torch.bfloat16, (6, 8))
    listed = torch.tensor([True, False, True, True, False, False])
    mask = listed[:, None]

    def good():
        o[0][listed] = xin[0][listed] * 2
    got, = fp.check(good, [xin], [o], written=mask)
    assert torch.equal(got[listed], x[listed] * 2)
    assert bool((fp._bits(got[~listed]) == fp.prefill_value(torch.bfloat16)).all())

    def writes_too_much():                                      # a row that is not on the list
        good()
        o[0][1, 3] = 0.0
    _raises(r'output 0: 1 elements outside the written part changed, first at \[1, 3\]', writes_too_much, [xin], [o], written=mask)

    def writes_too_little():                                    # a listed row left out
        o[0][listed] = xin[0][listed] * 2
        o[0][3, 7] = torch.tensor(fp.prefill_value(torch.bfloat16), dtype=torch.int16).view(torch.bfloat16)
    _raises(r'output 0: 1 elements the contract writes were not written, first at \[3, 7\]', writes_too_little, [xin], [o], written=mask)
    # a mask per output, None = the whole tensor
    o2 = fp.out((6,), torch.int32, CPU)

    def two():
        good()
        o2[0].copy_(torch.arange(6, dtype=torch.int32))
    fp.check(two, [xin], [o, o2], written=[mask, None])
    _raises('output 1: 3 elements the contract writes were not written', lambda: good(), [xin], [o, o2],
            written=[mask, listed])


def test_open_elements_and_scratch():
    """a (must, may) pair leaves some elements open; a SCRATCH output is checked at its guard bands only"""
    xin, o, x = _case(torch.float32, (4, 8))
    must = torch.zeros(4, 8, dtype=torch.bool); must[:, :5] = True
    may = torch.zeros(4, 8, dtype=torch.bool); may[:, :6] = True            # column 5: written or not (a thread stores two pixels)
    ws = fp.out((64,), torch.uint8, CPU)
    flat, start, n = _flat(ws)

    def run(cols=6, scratch_to=10):
        o[0][:, :cols] = xin[0][:, :cols]
        flat[start:start + scratch_to] = 1
    fp.check(run, [xin], [o, ws], written=[(must, may), fp.SCRATCH])
    fp.check(lambda: run(5), [xin], [o, ws], written=[(must, may), fp.SCRATCH])
    _raises('output 0: 4 elements outside the written part changed', lambda: run(7), [xin], [o, ws], written=[(must, may), fp.SCRATCH])
    _raises('output 0: 4 elements the contract writes were not written', lambda: run(4), [xin], [o, ws], written=[(must, may), fp.SCRATCH])
    _raises('output 1: the guard band after the tensor was written', lambda: run(6, 65), [xin], [o, ws], written=[(must, may), fp.SCRATCH])
