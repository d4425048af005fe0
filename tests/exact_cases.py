"""Operands, float64 reference and exactness budget of the bit-exact kernel tests.  (Not a test module: test_exact_cases_cpu.py shows on
the host that every case is sound, test_gpu_exact.py runs the HIP kernels on them and demands equality.)

The tolerance tests feed Gaussian operands, so a result depends on the fp32 summation order and can only be compared within a share of
the map's maximum.  Here every operand sits on a power-of-two grid coarse enough that EVERY partial sum of an accumulation, in any
order, is an integer multiple of the layer's quantum below 2^24 of them: fp32 adds them without rounding, the summation order drops out,
and the only roundings left are the 16-bit stores.  The reference is float64 with one round-to-nearest-even (fp16: after the clamp to
+-65504) at each place the kernel under test stores a 16-bit value.

  recipe          x                  w                   bias, residual   quantum of the sum
  coarse (bf16)   i/8,  |i| <= 8     j/64,  |j| <= 4     k/8, |k| <= 8    2^-9
  fine   (fp16)   i/32, |i| <= 32    j/256, |j| <= 16    k/8, |k| <= 8    2^-13
  chain           i/8,  |i| <= m     +-1 (first: +-2^-3 / x's quantum)   k/8   2^-3 in every layer
  the edges of fp16, on the recipes above (single layers: edge_scales; chains: EDGE_CHAINS; the table in front of EDGE_SINGLES has the rest):
  big  (both)     the recipe's       the recipe's x 2^s  k 2^12; i 32, |i| <= 2047 (bf16: i 256, |i| <= 255)   the recipe's x 2^s
  subw (fp16)     the fine recipe's  fine x 2^-14        (k/8) 2^-14                                           2^-27
  subx (fp16)     i 2^-24, |i| <= 32 fine x 2^5          (k/8) 2^-14                                           2^-27
  chain big, sub  x 2^xpow           +-2^p_i in layer i  k quanta of the layer's sums                          2^-3 x 2^(xpow + p_0 + .. + p_i)

(The coarse recipe under fp16 would round almost nothing: 11 significant bits hold nearly every sum.)  In a fused chain the quantum of a
layer's input is the quantum of the sums before it -- rounding a multiple of q to 16 bits leaves a multiple of q -- so the weights
are +-1 times a power of two: dense, and every further layer multiplies the quantum count only by its fan-in.  The power of the first
layer puts every layer's sums on the bias grid, 2^-3: a bias is then at most 8 quanta, a minor term, and no channel is alive or dead by its
bias alone (with biases of the size of the sums a one-channel output behind a ReLU is zero nearly everywhere).  The size m of x decides
which stores of the chain a case exercises: a store is rounded only where its sums overflow the significand, each layer adds several
bits, and a store more than five bits over has too few ties.  A deep chain therefore comes in variants (overflowing_x, Case.covers):
the plain case for its last stores, `_early` for its first; NOT_EXERCISED names the fp16 first stores that no case can reach inside the
budget.

Budget: for every accumulation of a case, sum |products| + |bias| + |residual| in units of that layer's quantum is at most 2^22 -- fp32
holds 2^24, the factor 4 is margin for a kernel that keeps more than one accumulator chain.  Single layers use the analytic worst case
K max|x| max|w|; chains run every layer on the absolute values of its (rounded) input in float64.  The bias and the residual are
checked on the grid of their own layer's sums, whatever power of two the regime put on it; a residual that sits on a finer grid than the
sums (Layer.rq: +-65504 = 2047 x 32) makes that grid the quantum the accumulation is counted in; and behind an fp16 store a grid finer
than 2^-24 is 2^-24 again (nothing finer is stored).
"""
import math
import zlib
from functools import lru_cache

import torch
import torch.nn.functional as F

BF, H16 = torch.bfloat16, torch.float16
DTYPES = (BF, H16)
IDS = {BF: 'bf16', H16: 'fp16'}
F16_MAX = 65504.0
F16_MIN_NORMAL, F16_SUB_Q = 2.0 ** -14, 2.0 ** -24       # below the first fp16 is subnormal, on multiples of the second
STORE_MUTANTS = ('noclamp', 'clamp', 'flush', 'trunc')
BUDGET_LOG2 = 22.0
RECIPE = {BF: dict(xm=8, xq=2.0 ** -3, wm=4, wq=2.0 ** -6), H16: dict(xm=32, xq=2.0 ** -5, wm=16, wq=2.0 ** -8)}
BIAS_Q = 2.0 ** -3


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32('/'.join(str(k) for k in key).encode()))


def grid(shape, m, q, g):
    """dense integers in [-m, m] times the power of two q, float64"""
    return torch.randint(-m, m + 1, tuple(shape), generator=g).double() * q


def signs(shape, q, g):
    """+-q, float64: the chain recipe's weights (cout, cin, kh, kw), as many +q as -q in every output channel's fan-in (one more -q
    where it is odd) in a random order: behind a ReLU every input is >= 0, and a surplus of one sign would decide the sign of the whole
    output channel -- alive everywhere or dead everywhere"""
    cout, k = shape[0], shape[1] * shape[2] * shape[3]
    order = torch.rand(cout, k, generator=g).argsort(dim=1)
    return ((order < k // 2).double() * 2 - 1).reshape(tuple(shape)) * q


def ftz(t):
    """fp16 subnormals flushed to zero"""
    return torch.where(t.abs() < F16_MIN_NORMAL, torch.zeros_like(t), t)


def r16(t, dt, model=None):
    """the kernels' 16-bit store on a tensor of exactly representable fp32 values held in any float type: fp16 clamps to +-65504, then
    round-to-nearest-even (also below 2^-14, where the quantum is 2^-24); returned in t's type.  model: a WRONG store, for
    test_edge_mutants_differ -- 'noclamp' (fp16 overflows to infinity), 'clamp' (bf16 with fp16's clamp), 'flush' (a subnormal result
    becomes zero), 'trunc' (below 2^-14 the value is cut towards zero instead of rounded)"""
    assert model in STORE_MUTANTS + (None,)
    v = t.float()
    known = ~t.isnan()                          # (behind a store without its clamp: infinity times zero)
    assert torch.equal(v.to(t.dtype)[known], t[known]), 'a value to be stored is not an fp32 value: the case is over its budget'
    if (dt == H16 and model != 'noclamp') or model == 'clamp':
        v = v.clamp(-F16_MAX, F16_MAX)
    out = v.to(dt).to(t.dtype)
    if model == 'flush':
        out = ftz(out)
    elif model == 'trunc':
        out = torch.where(t.abs() < F16_MIN_NORMAL, torch.trunc(t.double() / F16_SUB_Q).to(t.dtype) * F16_SUB_Q, out)
    return out


class Layer:
    """One accumulation and what the kernel does with it: conv(w, stride, pad) over the (2x nearest-upsampled if in_up) input + bias
    + residual ('same' size or stored at half size and nearest-upsampled), ReLU if act, one 16-bit store unless f32, then a max-pool
    (k, stride, pad) of the stored values.  wq: the quantum of the weights.  rq: the quantum of the residual where it is not on the
    grid of the sums (a residual at +-65504 lies on 32); the accumulation then counts in the finer of the two."""

    def __init__(self, w, b, wq, stride=1, pad=0, act=1, f32=False, in_up=0, pool=None, res=None, rq=None):
        self.w, self.b, self.wq, self.stride, self.pad, self.act, self.f32, self.in_up, self.pool, self.res, self.rq = w, b, wq, stride, pad, act, f32, in_up, pool, res, rq

    def but(self, **kw):
        """a copy with some fields replaced"""
        f = dict(w=self.w, b=self.b, wq=self.wq, stride=self.stride, pad=self.pad, act=self.act, f32=self.f32, in_up=self.in_up, pool=self.pool,
                 res=self.res, rq=self.rq)
        f.update(kw)
        return Layer(**f)

    def accumulate(self, t, absolute=False, flush=False):
        """flush: the WRONG multiply of test_edge_mutants_differ -- the 16-bit operands (input, weights, residual) lose their fp16
        subnormals before it"""
        ab = (lambda v: v.abs()) if absolute else (ftz if flush else (lambda v: v))
        if self.in_up:
            t = F.interpolate(t, scale_factor=2.0, mode='nearest')
        bias = (self.b.abs() if absolute else self.b).to(t.dtype) if self.b is not None else None          # (fp32 in the kernels)
        y = F.conv2d(ab(t), ab(self.w).to(t.dtype), bias, stride=self.stride, padding=self.pad)
        if self.res is not None:
            r = ab(self.res[:t.shape[0]]).to(t.dtype)
            y = y + (r if r.shape[-2:] == y.shape[-2:] else F.interpolate(r, size=y.shape[-2:], mode='nearest'))
        return y

    def forward(self, t, dt, mutant=None):
        """-> (what the next layer reads, the 16-bit values stored before the pool or None, the sums behind the activation they were rounded from).
        mutant: None | 'operands' (accumulate's flush) | 'input' (only the layer's input loses its subnormals) | a store model of r16
        ('clamp' on an fp32 output clamps that)"""
        if mutant == 'input':
            t = ftz(t)
        y = sums = self.accumulate(t, flush=mutant == 'operands')
        if self.act:
            y = sums = F.relu(y)
        stored = None
        if not self.f32:
            y = stored = r16(y, dt, mutant if mutant in STORE_MUTANTS else None)
        elif mutant == 'clamp':
            y = y.clamp(-F16_MAX, F16_MAX)
        if self.pool:
            y = F.max_pool2d(y, *self.pool)
        return y, stored, sums


class Case:
    def __init__(self, family, name, dt, x, xq, layers, keep=None):
        """x (N,C,H,W) float64 on the grid xq; keep: how many images (from the end of the batch) the host checks and the GPU test
        compares -- the kernels run the whole batch."""
        self.family, self.name, self.dt, self.x, self.xq, self.layers = family, name, dt, x, xq, layers
        self.keep = keep or x.shape[0]
        self.id = f'{family}/{name}/{IDS[dt]}'
        # the stored layers (indices into the 16-bit stores, in order) whose rounding this case is there to exercise: each must meet the
        # share conditions of test_exact_cases_cpu.py on its own.  Default: the last store
        self.covers = None
        # None | 'big' | 'subw' | 'subx' | 'sub' (a chain): the edge of fp16 the case sits on
        self.regime = None

    def named_operands(self):
        """the 16-bit operand tensors a sub regime names: their non-zero values are fp16 subnormals"""
        if self.regime in ('subw', 'subx'):
            return [self.layers[0].w] if self.regime == 'subw' else [self.x]
        if self.regime == 'sub':                 # a chain: x or the first layer's weights, whichever the case put below 2^-14
            return [t for t in (self.x, self.layers[0].w) if float(t.abs().max()) < F16_MIN_NORMAL]
        return []

    def kept(self, t):
        return t[t.shape[0] - self.keep:]

    def with_(self, x=None, layers=None):
        c = Case(self.family, self.name, self.dt, self.x if x is None else x, self.xq, self.layers if layers is None else layers, None)
        c.keep = min(self.keep, c.x.shape[0])
        c.covers, c.regime = self.covers, self.regime
        return c

    def reference(self, ftype=torch.float64, images=None, sums=False, mutant=None):
        """-> (final output NCHW in ftype, [stored 16-bit tensors]) over the kept images (or `images`, a slice of the batch); with
        sums=True also the unrounded sums of the stored layers.  mutant: (layer index, what Layer.forward does wrong there)"""
        sl = images if images is not None else slice(self.x.shape[0] - self.keep, None)
        t = self.x[sl].to(ftype)
        stored, unrounded = [], []
        for i, L in enumerate(self.layers):
            L = _sliced(L, sl)
            t, s, y = L.forward(t, self.dt, mutant[1] if mutant and mutant[0] == i else None)
            if s is not None:
                stored.append(s)
                unrounded.append(y)
        return (t, stored, unrounded) if sums else (t, stored)

    def budget(self):
        """-> (log2 of the largest accumulation in quanta over the layers, the quantum of the final sums).  Checks on the way that every
        operand sits on its grid."""
        sl = slice(self.x.shape[0] - self.keep, None)
        q = self.xq
        _on_grid(self.x, q, 'x')
        t = self.x[sl]
        worst = 0.0
        for i, L0 in enumerate(self.layers):
            L = _sliced(L0, sl)
            _on_grid(L.w, L.wq, f'w{i}')
            _on_grid(t, q, f'the input of layer {i}')          # (a store clamped to 65504 = 2047 x 32 stays on grids of 32 and finer only)
            q = q * L.wq
            if L.b is not None:
                _on_grid(L.b, q, f'bias{i}')
            if L0.res is not None:
                if L.rq is not None:
                    q = min(q, L.rq)
                _on_grid(L0.res, q, f'residual{i}')
                assert torch.equal(L0.res.to(self.dt).double(), L0.res), f'residual{i} is not a value of the storage type'
            if len(self.layers) == 1:          # the analytic worst case: every product at the operands' maxima
                k = L.w.shape[1] * L.w.shape[2] * L.w.shape[3]
                total = k * float(self.x.abs().max()) * float(L.w.abs().max()) + (float(L.b.abs().max()) if L.b is not None else 0.0) \
                    + (float(L0.res.abs().max()) if L0.res is not None else 0.0)
            else:                               # the data: this layer on the absolute values of its rounded input
                total = float(L.accumulate(t, absolute=True).max())
            worst = max(worst, total / q)
            if len(self.layers) > 1:
                t = L.forward(t, self.dt)[0]
            if self.dt == H16 and not L.f32:
                q = max(q, F16_SUB_Q)               # (whatever fp16 stores is a multiple of 2^-24: a finer grid ends at the store)
        return math.log2(max(worst, 1.0)), q


def _sliced(L, sl):
    return L if L.res is None else L.but(res=L.res[sl])


def _on_grid(t, q, what):
    assert torch.equal(torch.round(t / q) * q, t), f'{what} is not on the grid {q}'


def shares(case, stored, sums):
    """Per 16-bit store of the case, in order (`stored` and `sums` of case.reference(sums=True)): (share of non-zero values, of values that
    needed a rounding, of exact ties, their number).  A fused kernel's first store is judged on its own: averaged with the later ones, a
    layer whose sums never overflow the significand -- a store the case cannot see at all -- would hide behind them."""
    out = []
    for s, y in zip(stored, sums):
        inexact = s != y
        mirror = 2 * y - s                      # RNE took the nearer neighbour: a tie iff the point as far on the other side is one too
        tie = inexact & (r16(mirror, case.dt) == mirror)
        out.append((float((s != 0).double().mean()), float(inexact.double().mean()), float(tie.double().mean()), s.numel()))
    return out


def covered(case):
    """the stored layers the case answers for (Case.covers; default: the last store)"""
    n = sum(1 for L in case.layers if not L.f32)
    return set(case.covers) if case.covers is not None else ({n - 1} if n else set())


# ---------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------
PRODUCT_STD = {BF: 0.02468, H16: 0.02146}                # of one product x w on the recipe of the storage type
BIG_RES = {BF: (255, 256.0), H16: (2047, 32.0)}          # a `big` residual: |i| <= m times q, all values of the storage type up to 65504
BIG_BIAS_Q = 4096.0                                      # a `big` bias: k 2^12, |k| <= 8 -- on every grid of sums in use, and at most half of 65504
REGIMES = ('big', 'subw', 'subx')


def edge_scales(regime, dt, fan_in):
    """-> (log2 of the factor on x, on the weights) of a single layer in an edge regime.  big: the sums' standard deviation stands at
    about 65504 (17 at a fan-in of 576).  subw: 2^-14 makes every weight of the fine recipe an fp16 subnormal and the sums of 576 products
    as well; a larger fan-in takes a smaller power, so that the sums stay below 2^-14.  subx: x on i 2^-24, and the weights times 2^5
    (less at a larger fan-in): the sums lie on 2^-27, three bits below the subnormal quantum -- one store in 8 is an exact tie."""
    over = max(0, math.floor(math.log2(math.sqrt(fan_in / 576.0))))
    if regime == 'big':
        return 0, round(math.log2(1.3 * F16_MAX / (math.sqrt(fan_in) * PRODUCT_STD[dt])))
    assert dt == H16, 'bf16 has no subnormals within reach: its exponent range is that of fp32'
    return {'subw': (0, -14 - over), 'subx': (-19, 5 - over)}[regime]


def big_residual(shape, dt, g):
    """a 16-bit residual for a `big` case: values of the storage type spread over +-65504 -- and in fp16 exactly +-65504 at one
    position in 50: a sum added to a residual that already sits at the limit must still clamp"""
    m, q = BIG_RES[dt]
    r = grid(shape, m, q, g)
    if dt == H16:
        at_limit = torch.rand(tuple(shape), generator=g) < 0.02
        sign = (torch.rand(tuple(shape), generator=g) < 0.5).double() * 2 - 1
        r = torch.where(at_limit, sign * F16_MAX, r)
    return r


def single(family, name, dt, n, cin, h, w, cout, k, stride, pad, act=1, f32=False, in_up=0, pool=False, res=None, keep=None, bias=True,
           wscale=None, salt=0, regime=None):
    """One conv layer on the recipe of its storage type.  res: None | 'same' | 'up' (stored at the output's half size, rounded up).
    wscale: per-cout powers of two folded into the weights (a frozen batch norm's scale).  regime: None | 'big' | 'subw' | 'subx'
    (edge_scales); the bias and the residual move with the grid of the sums."""
    rc = RECIPE[dt]
    g = seeded(family, name, *([salt] if salt else []))
    xs, ws = edge_scales(regime, dt, cin * k * k) if regime else (0, 0)
    x = grid((n, cin, h, w), rc['xm'], rc['xq'], g) * 2.0 ** xs
    wgt = grid((cout, cin, k, k), rc['wm'], rc['wq'], g) * 2.0 ** ws
    xq, wq = rc['xq'] * 2.0 ** xs, rc['wq'] * 2.0 ** ws
    if wscale is not None:
        wgt = wgt * wscale[:, None, None, None]
        wq = wq * float(wscale.min())
    b = grid((cout,), 8, BIG_BIAS_Q if regime == 'big' else BIAS_Q * 2.0 ** (xs + ws), g) if bias else None
    ho = ((h << in_up) + 2 * pad - k) // stride + 1
    wo = ((w << in_up) + 2 * pad - k) // stride + 1
    r, rq = None, None
    if res:
        shape = (n, cout, ho, wo) if res == 'same' else (n, cout, (ho + 1) // 2, (wo + 1) // 2)
        if regime == 'big':
            r, rq = big_residual(shape, dt, g), BIG_RES[dt][1]
        else:
            r = grid(shape, 8, BIAS_Q, g) * 2.0 ** (xs + ws)
    L = Layer(wgt, b, wq, stride, pad, act, f32, in_up, (2, 2, 0) if pool else None, r, rq)
    case = Case(family, name, dt, x, xq, [L], keep)
    case.regime = regime
    return case


CHAIN_X = {BF: (2, 2.0 ** -1), H16: (8, 2.0 ** -3)}      # |i| <= 2 halves | |i| <= 8 eighths: a chain's last store keeps a few bits more than it rounds to


def overflowing_x(dt, fan_in, bits_over):
    """the x grid (|i| <= m eighths) with which the sums of a chain's FIRST layer (+-1 weights over fan_in inputs: standard deviation
    sqrt(fan_in) m / sqrt(3) quanta) stand bits_over bits above the significand of the storage type (8 | 11 bits).  One bit over: about
    20 % of that store needs a rounding, 11 % are ties.  Each further layer adds log2(0.6 sqrt(fan-in)) bits, and a store more than
    five bits over has too few ties -- so one case cannot exercise every store of a deep chain, and a chain comes in variants: the
    plain one for its last stores, `_early` for its first."""
    sigma = 2.0 ** ((8 if dt == BF else 11) + bits_over)
    m = max(1, math.ceil(sigma * math.sqrt(3) / math.sqrt(fan_in)))
    assert m < (256 if dt == BF else 1024), 'x would not fit the storage type'
    return m, BIAS_Q


def chain(family, name, dt, n, cin, h, w, specs, keep=None, res_last=None, xgrid=None, first=None, covers=None, xpow=0, powers=None, regime=None, salt=0):
    """specs: per layer (cout, k, stride, pad, act, f32, in_up, pool) with weights +-1, the first layer's +-2^-3 / x's quantum; x:
    integers |i| <= xgrid[0] times xgrid[1] (default CHAIN_X of the storage type).  first: a RECIPE entry whose weight grid the first layer takes instead.
    res_last: None | 'x' (the input itself) | 'sep' (a separate tensor on the k/8 grid) added in the last layer.
    xpow, powers: x and layer i's weights take the factors 2^xpow and 2^powers[i] (the edge regimes); every bias, and a separate residual,
    moves with the grid of its sums -- a `big` case's separate residual is big_residual's."""
    g = seeded(family, name, *([salt] if salt else []))
    xm, xq = xgrid or CHAIN_X[dt]
    x = grid((n, cin, h, w), xm, xq, g) * 2.0 ** xpow
    powers = powers or [0] * len(specs)
    layers, c, total, qlog = [], cin, xpow, math.log2(xq) + xpow          # (qlog: log2 of the quantum of the sums)
    for i, (cout, k, stride, pad, act, f32, in_up, pool) in enumerate(specs):
        if i == 0 and first is not None:
            wgt, wq = grid((cout, c, k, k), first['wm'], first['wq'], g), first['wq']
        else:
            wq = BIAS_Q / xq if i == 0 else 1.0          # every layer's sums on the bias grid, 2^-3: a bias is at most 8 quanta of them
            wgt = signs((cout, c, k, k), wq, g)
        wgt, wq, total = wgt * 2.0 ** powers[i], wq * 2.0 ** powers[i], total + powers[i]
        qlog += math.log2(wq)
        b = grid((cout,), 8, BIAS_Q, g) * 2.0 ** total
        if cout == 1:
            b = b.abs()                            # (a single output channel with a negative bias would be dead behind its ReLU)
        r, rq = None, None
        if i == len(specs) - 1 and res_last:
            if res_last == 'x':
                r, rq = x, xq * 2.0 ** xpow
            elif regime == 'big':
                r, rq = big_residual((n, cout, h, w), dt, g), BIG_RES[dt][1]
            else:
                r = grid((n, cout, h, w), 8, BIAS_Q, g) * 2.0 ** (max(total, -21) if dt == H16 else total)      # (16-bit: k 2^-24 at the finest)
        layers.append(Layer(wgt, b, wq, stride, pad, act, f32, in_up, pool, r, rq))
        c = cout
        if dt == H16 and not f32 and qlog < -24:    # (fp16 stores multiples of 2^-24: the next layer's grid starts from there)
            total, qlog = total - 24 - qlog, -24
    case = Case(family, name, dt, x, xq * 2.0 ** xpow, layers, keep)
    case.covers, case.regime = covers, regime
    return case


# the small rows of tests/test_gpu_kernels.py CONV_CASES: name -> (n, cin, h, w, cout, k, stride, pad, options)
IGEMM = {
    'stem7x7': (2, 3, 67, 45, 64, 7, 2, 3, {'salt': 1}),
    '3x3_s2': (2, 64, 26, 30, 64, 3, 2, 1, {}),
    'cin32': (1, 32, 30, 30, 32, 3, 1, 1, {}),
    'cin16_1x1': (1, 16, 30, 31, 16, 1, 1, 0, {'salt': 1}),
    'ragged_m': (3, 64, 5, 3, 192, 3, 1, 1, {}),
    'residual': (2, 64, 18, 22, 256, 1, 1, 0, {'res': 'same'}),
    'res_upsample': (2, 64, 20, 24, 256, 1, 1, 0, {'res': 'up', 'act': 0}),
    'in_upsample': (1, 64, 12, 14, 32, 3, 1, 1, {'in_up': 1}),
    'cls_f32': (2, 256, 13, 13, 9, 3, 1, 1, {'f32': True, 'act': 0}),
    'reg_f32': (1, 256, 7, 7, 36, 3, 1, 1, {'f32': True, 'act': 0}),
    'gauss_out': (1, 16, 40, 40, 1, 1, 1, 0, {'f32': True, 'act': 1}),
    'deep_k': (1, 512, 9, 9, 512, 3, 1, 1, {}),
    'pool_generic': (3, 32, 20, 24, 64, 3, 1, 1, {'pool': True}),
    'pool_generic_first': (2, 3, 36, 40, 64, 3, 1, 1, {'pool': True}),
}
DMA = {   # the LDS-DMA ring kernels need their whole batch (128 pixel tiles of 256); one image is compared
    'dma64': (2, 64, 128, 128, 64, 3, 1, 1, {}),
    'dma128': (2, 64, 128, 128, 128, 3, 1, 1, {}),
    'dma256': (2, 64, 128, 128, 256, 3, 1, 1, {}),
    'dma_ragged': (1, 64, 181, 182, 192, 3, 1, 1, {}),
    'dma_in_up': (1, 64, 91, 90, 192, 3, 1, 1, {'in_up': 1}),      # 182 x 180 output: 128 pixel tiles, the last ragged; conv_dma_kernel<256,256>
    'dma_res_up': (2, 64, 128, 128, 256, 1, 1, 0, {'res': 'up', 'act': 0}),
    'pool_dma64': (2, 64, 128, 128, 64, 3, 1, 1, {'pool': True}),
}
SPLITK = [   # tests/test_gpu_kernels.py test_conv2d_splitk_parity (the last image is compared): n, cin, h, w, cout, k, stride, act
    (4, 512, 25, 25, 512, 3, 1, 1), (2, 512, 50, 50, 512, 3, 2, 1), (3, 256, 64, 64, 256, 3, 2, 1), (4, 256, 13, 13, 256, 3, 2, 0),
    (1, 256, 25, 25, 256, 3, 1, 0), (2, 320, 9, 11, 200, 3, 1, 1),
]
C1X1 = [   # tests/test_gpu_kernels.py C1X1_CASES: n, cin, h, w, cout, stride, res, act
    (2, 64, 40, 52, 256, 1, 'same', 1), (2, 256, 40, 52, 64, 1, '', 1), (3, 256, 33, 47, 512, 2, '', 0), (1, 1024, 13, 17, 256, 1, 'up', 0),
    (2, 512, 7, 9, 2048, 1, 'same', 1), (1, 2048, 5, 5, 512, 1, '', 1), (1, 128, 5, 7, 192, 1, 'same', 1), (2, 128, 61, 67, 512, 1, 'same', 1),
    (1, 64, 30, 31, 128, 1, 'up', 1),
]
HALO = [   # n, cin, h, w, cout, pool
    (2, 64, 30, 44, 96, True), (2, 192, 40, 70, 128, True), (2, 128, 26, 38, 128, True), (2, 256, 13, 13, 256, False), (1, 256, 50, 50, 256, False),
    (2, 64, 48, 80, 128, False), (1, 256, 32, 32, 512, False), (2, 512, 16, 16, 512, False),
    (2, 64, 33, 31, 136, False), (2, 192, 33, 31, 264, False),          # the ragged cout tiles of the footprint test
]
MAC = [(5, 128, 32, 32, 512, True, True), (3, 64, 16, 16, 512, False, False), (2, 64, 40, 24, 256, False, True)]   # n, cin, h, w, cout, pool, store
THIN_OUT = [(cout, cin, h, w) for cout in (1, 9, 36) for cin, h, w in ((128, 48, 48), (64, 50, 77))]
THIN3X3 = [(2, 37, 45, 32, 0), (1, 103, 16, 16, 0), (3, 7, 70, 32, 0), (1, 51, 33, 16, 0), (2, 19, 23, 32, 1), (1, 52, 8, 32, 1), (1, 3, 40, 32, 1)]   # n, h, w, cout, up
VGG_STEM = [(3, 16, 16), (1, 16, 32), (2, 32, 48)]
GLN_STEM = [(1, 1, 1), (1, 7, 9), (3, 37, 51), (2, 130, 66)]
GAUSS_TAIL = [(1, 1, 1), (1, 1, 63), (1, 37, 41)]
GAUSS_SUBNET = [(1, 1, 1), (1, 3, 57), (1, 7, 29), (2, 19, 23), (2, 64, 15)]
BNECK = [(2, 256, 64, 56, 56, False), (1, 64, 64, 37, 51, True), (2, 512, 128, 100, 100, False), (1, 512, 128, 5, 9, False),
         (2, 1024, 256, 50, 50, False), (1, 1024, 256, 15, 29, False)]   # tests/test_gpu_kernels.py BNECK_CASES


@lru_cache(maxsize=None)
def gln_scale():
    """a frozen batch norm whose scales are powers of two: folded into a grid weight they stay exact"""
    return 2.0 ** torch.randint(-1, 2, (64,), generator=seeded('gln_scale')).double()


def subnet_specs(act):
    # 64 -(3x3 over the 2x upsample)-> 32 -> 32 -> 16 -(1x1)-> 16 -> 1 (f32)
    return [(32, 3, 1, 1, 1, False, 1, None), (32, 3, 1, 1, 1, False, 0, None), (16, 3, 1, 1, 1, False, 0, None),
            (16, 1, 1, 0, 1, False, 0, None), (1, 1, 1, 0, act, True, 0, None)]


def tail_specs(act=1):
    # (integers TAIL_X times the fine recipe's weights for both types -- bf16 holds both: 16 coarse products would rarely need a rounding)
    return [(16, 1, 1, 0, 1, False, 0, None), (1, 1, 1, 0, act, True, 0, None)]


def bneck_specs(p):
    return [(p, 1, 1, 0, 1, False, 0, None), (p, 3, 1, 1, 1, False, 0, None), (4 * p, 1, 1, 0, 1, False, 0, None)]


TAIL_X = {BF: (32, 1.0), H16: (256, 1.0)}                # (16 products have to overflow 8 | 11 significant bits)
BNECK_X = {BF: (1, 2.0 ** -1), H16: (4, 2.0 ** -2)}     # (three layers of fan-in 1024, 2304, 256 behind it; fp16 at Cin = 64: |i| <= 32, or 11 bits hold every sum)


def subnet_variants(dt):
    """-> [(name suffix, x grid, stored layers covered)].  fp16: x large enough for the second store to overflow 11 bits; a first store
    that overflows them would put the last layer's sums past the 2^22 budget (measured: 2^22.6), so no fp16 case exercises it."""
    if dt == BF:
        return [('', CHAIN_X[BF], (1, 2, 3)), ('_early', overflowing_x(BF, 576, 1.0), (0, 1))]
    return [('', overflowing_x(H16, 576, -2.5), (1, 2, 3))]


def bneck_variants(dt, cin, p):
    """-> [(name suffix, x grid, stored layers covered)].  fp16 at P = 256: a first store that overflows 11 bits needs 2^23.8 quanta in
    the third layer -- over the budget, so no case exercises it; at P = 128 it fits with 0.3 bits over (2^21.9)."""
    if dt == BF:
        return [('', BNECK_X[BF], (1, 2) if p == 256 else (2,)), ('_early', overflowing_x(BF, cin, 1.0), (0,) if p == 256 else (0, 1))]
    if p == 64:
        return [('', (32, 2.0 ** -5) if cin == 64 else BNECK_X[H16], (2,)), ('_early', overflowing_x(H16, cin, 1.0), (0, 1))]
    if p == 128:
        return [('', overflowing_x(H16, cin, -3.5), (1, 2)), ('_early', overflowing_x(H16, cin, 0.3), (0,))]
    return [('', BNECK_X[H16], (1, 2))]


# stored layers that no case can exercise inside the budget (see the two functions above): (family, type, planes or None) -> layers
NOT_EXERCISED = {('gauss_subnet', H16, None): {0}, ('bneck', H16, 256): {0}}


def builders():
    """-> {case id: builder}: every case of test_gpu_exact.py that runs from this table, built on demand (`case(id)` caches)"""
    out = {}

    def add(family, name, dt, fn):
        out[f'{family}/{name}/{IDS[dt]}'] = fn
    for dt in DTYPES:
        add('anchor', 'pointwise_8x8', dt, lambda dt=dt: single('anchor', 'pointwise_8x8', dt, 1, 64, 8, 8, 64, 1, 1, 0, act=0, f32=True))
        add('anchor', 'centre_tap_48x48', dt, lambda dt=dt: centre_tap(single('anchor', 'centre_tap_48x48', dt, 1, 64, 48, 48, 64, 3, 1, 1, act=0, f32=True)))
        for name, c in IGEMM.items():
            add('igemm', name, dt, lambda dt=dt, name=name, c=c: single('igemm', name, dt, *c[:8], **_opts(c[8])))
        for name, c in DMA.items():
            add('dma', name, dt, lambda dt=dt, name=name, c=c: single('dma', name, dt, *c[:8], keep=1, **_opts(c[8])))
        for (n, cin, h, w, cout, k, stride, act) in SPLITK:
            for f32 in (False, True):
                for res in (None, 'same'):
                    name = f'{cin}x{h}x{w}-{cout}s{stride}' + ('_f32' if f32 else '') + ('_res' if res else '')
                    add('splitk', name, dt, lambda dt=dt, name=name, a=(n, cin, h, w, cout, k, stride, k // 2), act=act, f32=f32, res=res:
                        single('splitk', name, dt, *a, act=act, f32=f32, res=res, keep=1))
        for (n, cin, h, w, cout, stride, res, act) in C1X1:
            name = f'{cin}x{h}x{w}-{cout}s{stride}{res}'
            add('conv1x1', name, dt, lambda dt=dt, name=name, a=(n, cin, h, w, cout, 1, stride, 0), act=act, res=res:
                single('conv1x1', name, dt, *a, act=act, res=res or None))
        for (n, cin, h, w, cout, pool) in HALO:
            name = f'{cin}x{h}x{w}-{cout}' + ('_pool' if pool else '')
            add('halo', name, dt, lambda dt=dt, name=name, a=(n, cin, h, w, cout, 3, 1, 1), pool=pool: single('halo', name, dt, *a, pool=pool))
        for tag, (hh, ww) in (('a', (21, 30)), ('b', (9, 14))):
            add('atlas', tag, dt, lambda dt=dt, tag=tag, hh=hh, ww=ww: single('atlas', tag, dt, 3, 128, hh, ww, 256, 3, 1, 1))
        for (cout, cin, h, w) in THIN_OUT:
            name = f'{cin}x{h}x{w}-{cout}'
            add('thin_out', name, dt, lambda dt=dt, name=name, a=(2, cin, h, w, cout, 3, 1, 1): single('thin_out', name, dt, *a, act=0, f32=True))
        for (n, h, w, cout, up) in THIN3X3:
            for act in (0, 1):
                name = f'{n}x{h}x{w}-{cout}' + ('_up' if up else '') + f'_act{act}'
                add('thin3x3', name, dt, lambda dt=dt, name=name, a=(n, 64 if up else 32, h, w, cout, 3, 1, 1), act=act, up=up:
                    single('thin3x3', name, dt, *a, act=act, in_up=up))
        for (n, h, w) in GLN_STEM:
            add('gln_stem', f'{n}x{h}x{w}', dt, lambda dt=dt, a=(n, h, w): gln_stem_case(dt, *a))
        for (n, h, w) in GAUSS_TAIL:
            add('gauss_tail', f'{n}x{h}x{w}', dt, lambda dt=dt, a=(n, h, w): chain('gauss_tail', f'{a[0]}x{a[1]}x{a[2]}', dt, a[0], 16, a[1], a[2], tail_specs(), xgrid=TAIL_X[dt], first=RECIPE[H16]))
        for (n, h, w) in GAUSS_SUBNET:
            for act in (0, 1):
                for sfx, xg, cov in subnet_variants(dt):
                    if sfx and n * h * w == 1:
                        continue                   # (a 2 x 2 output shows nothing of a first store four layers back: the plain case stays)
                    name = f'{n}x{h}x{w}_act{act}{sfx}'
                    add('gauss_subnet', name, dt, lambda dt=dt, name=name, a=(n, h, w), act=act, xg=xg, cov=cov:
                        chain('gauss_subnet', name, dt, a[0], 64, a[1], a[2], subnet_specs(act), xgrid=xg, covers=cov))
        for (n, cin, p, h, w, sep) in BNECK:
            for sfx, xg, cov in bneck_variants(dt, cin, p):
                name = f'{cin}-{p}x{h}x{w}' + ('_sep' if sep else '') + sfx
                add('bneck', name, dt, lambda dt=dt, name=name, a=(n, cin, h, w), p=p, sep=sep, xg=xg, cov=cov:
                    chain('bneck', name, dt, *a, bneck_specs(p), keep=1, res_last='sep' if sep else 'x', xgrid=xg, covers=cov))
    for (n, cin, h, w, cout, pool, store) in MAC:
        name = f'{cin}x{h}x{w}-{cout}' + ('_pool' if pool else '') + ('' if store else '_nostore')
        add('mac', name, BF, lambda name=name, a=(n, cin, h, w, cout, 3, 1, 1): single('mac', name, BF, *a))
    for (n, h, w) in VGG_STEM:
        add('vgg_stem', f'{n}x{h}x{w}', BF, lambda a=(n, h, w): vgg_stem_case(*a))
    return out


def _opts(o):
    return dict(act=o.get('act', 1), f32=o.get('f32', False), in_up=o.get('in_up', 0), pool=o.get('pool', False), res=o.get('res'), salt=o.get('salt', 0))


def centre_tap(case):
    """a 3x3 layer whose weights are zero off the centre tap: the pointwise conv of the anchor, for a kernel that only runs 3x3"""
    w = case.layers[0].w
    keep = torch.zeros_like(w)
    keep[:, :, 1, 1] = w[:, :, 1, 1]
    case.layers[0].w = keep
    return case


def vgg_stem_case(n, h, w, name=None, powers=None, regime=None):
    """conv1_1 (3 -> 64, +-1) + ReLU stored, conv1_2 (64 -> 64, +-1) + ReLU stored, MaxPool2d(2, 2); x large enough for conv1_1's 27
    products to stand one bit over bf16's significand -- conv1_2 then stands four over: one case exercises both stores"""
    return chain('vgg_stem', name or f'{n}x{h}x{w}', BF, n, 3, h, w, [(64, 3, 1, 1, 1, False, 0, None), (64, 3, 1, 1, 1, False, 0, (2, 2, 0))],
                 xgrid=overflowing_x(BF, 27, 1.0), covers=(0, 1), powers=powers, regime=regime)


def gln_stem_case(dt, n, h, w, regime=None):
    """conv 7x7 / 2 with a power-of-two frozen batch norm folded into the weights + ReLU, stored, then MaxPool2d(3, 2, 1) (exact)"""
    # (big: no scale above 1 -- a channel at twice the regime's size is saturated nearly everywhere behind the 3 x 3 pool, and shows nothing)
    scale = gln_scale().clamp(max=1.0) if regime == 'big' else gln_scale()
    c = single('gln_stem', f'{n}x{h}x{w}' + (f'_{regime}' if regime else ''), dt, n, 3, h, w, 64, 7, 2, 3, wscale=scale, regime=regime)
    c.layers[0].pool = (3, 2, 1)
    c.scale = scale
    c.wt = c.layers[0].w / c.scale[:, None, None, None]          # what the model holds: the weight before the fold
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# the edges of fp16: saturated stores (`big`) and subnormal operands and stores (`subw`, `subx`; a chain: `sub`)
#
#   regime   x                     w                          bias                  residual (16-bit)                 what it shows
#   big      the recipe's          the recipe's times 2^s     k 2^12, |k| <= 8      fp16: i 32, |i| <= 2047, one in   fp16 stores clamp at +-65504, bf16 and fp32
#            (fp16 and bf16)       (edge_scales: 17 at a      (on every grid of     50 exactly +-65504; bf16: i 256,  stores do not
#                                  fan-in of 576)             sums in use)          |i| <= 255
#   subw     the fine recipe's     the fine recipe's times    (k/8) 2^-14           (k/8) 2^-14: multiples of 2^-24   subnormal weights count at their value; a store
#            (fp16)                2^-14: all subnormal                                                                rounds to nearest even on the 2^-24 grid
#   subx     i 2^-24, |i| <= 32:   the fine recipe's times    (k/8) 2^-14           (k/8) 2^-14                       the same for subnormal activations
#            all subnormal         2^5
#   chain    layer i's +-1 weights take the factor 2^p_i and x the factor 2^xpow (EDGE_CHAINS); every bias is k quanta of its layer's sums
#
# A power of two on the weights changes no product's exactness and no count of quanta: the budget of a scaled single layer is that of the
# plain one.  In a chain the clamp does not commute with the scale, and two things follow.  (1) 65504 = 2047 x 32 lies on the grids of 32
# and finer only, so an fp16 store that saturates has a quantum of at most 32 and therefore sums of 2^11 quanta and more: a `big` chain
# starts from an x of overflowing_x's size, on the grid 2^-3 x 2^8 = 32 (an identity residual is then on the grid of the last sums).
# (2) Behind a store that saturates in part, the next layer's power brings the sums back to about 65504, on a finer grid; with it every
# store of the three chains saturates in part inside the budget (measured: bneck at P = 256 2^21.8, the subnet 2^20.2), so NOT_EXERCISED_EDGE
# is empty.  A `sub` chain keeps every store below 2^-14: whatever fp16 stores is a multiple of 2^-24, so each layer's power of about
# 2^-3 puts its sums on 2^-27 again -- three bits to round, one store in eight an exact tie, at a budget below 2^18.
# ---------------------------------------------------------------------------------------------------------------------------------
# family -> [(existing case name, regimes: B = big in both types, w = subw, x = subx)]
EDGE_SINGLES = {
    'igemm': [('3x3_s2', 'Bwx'), ('residual', 'Bwx'), ('res_upsample', 'Bw'), ('in_upsample', 'Bx'), ('pool_generic', 'Bw'), ('cls_f32', 'B')],
    'dma': [('dma128', 'Bwx'), ('dma_res_up', 'Bw')],
    'splitk': [('512x25x25-512s1', 'Bwx'), ('512x25x25-512s1_res', 'Bw')],
    'conv1x1': [('256x33x47-512s2', 'Bwx'), ('64x40x52-256s1same', 'Bwx'), ('64x30x31-128s1up', 'Bx')],
    'halo': [('64x48x80-128', 'Bwx'), ('256x13x13-256', 'Bwx'), ('64x30x44-96_pool', 'Bw')],
    'atlas': [('a', 'Bwx')],
    'thin_out': [('128x48x48-9', 'Bwx')],
    'thin3x3': [('2x37x45-32_act0', 'Bwx'), ('2x19x23-32_up_act1', 'Bx')],
    'gln_stem': [('3x37x51', 'Bwx')],
}
EDGE_MAC, EDGE_VGG_STEM = (2, 64, 40, 24, 256), (1, 16, 32)       # bf16 only: `big`
# chain family -> {(planes or None, regime, type): (x grid, xpow, powers)}; every case covers all of its stores
EDGE_CHAINS = {
    'gauss_tail': {(None, 'big', H16): (TAIL_X[H16], 0, [12, -17]), (None, 'big', BF): (TAIL_X[BF], 0, [15, -18]),
                   (None, 'sub', H16): (TAIL_X[H16], -24, [4, 14])},
    'gauss_subnet': {(None, 'big', H16): (overflowing_x(H16, 576, 0.0), 8, [0, -2, -3, 0, -17]), (None, 'big', BF): (CHAIN_X[BF], 14, [0, -3, -3, -2, -17]),
                     (None, 'sub', H16): (overflowing_x(H16, 576, 0.0), 0, [-24, -3, -3, -2, 14])},
    'bneck': {(64, 'big', H16): (overflowing_x(H16, 64, 0.0), 8, [0, -3, -1]), (64, 'big', BF): (BNECK_X[BF], 16, [0, -4, -2]),
              (128, 'big', H16): (overflowing_x(H16, 512, 0.0), 8, [0, -3, -2]), (128, 'big', BF): (BNECK_X[BF], 15, [0, -4, -3]),
              (256, 'big', H16): (overflowing_x(H16, 1024, 0.0), 8, [0, -4, -2]), (256, 'big', BF): (BNECK_X[BF], 15, [0, -5, -3]),
              (64, 'sub', H16): (overflowing_x(H16, 64, -1.5), -21, [-2, -4, -3]), (128, 'sub', H16): (overflowing_x(H16, 512, -1.5), -21, [-2, -4, -3]),
              (256, 'sub', H16): (overflowing_x(H16, 1024, -1.5), -21, [-2, -4, -3])},
}
EDGE_TAIL, EDGE_SUBNET, EDGE_BNECK = (1, 37, 41), (2, 19, 23), [(1, 64, 64, 37, 51, True), (1, 512, 128, 5, 9, False), (1, 1024, 256, 15, 29, False)]
VGG_STEM_BIG = [10, -3]
EDGE_TAIL_SALT = {('big', H16): 2, ('big', BF): 1, ('sub', H16): 1}          # (the seeds with which the one output channel is alive at pixel (0, 0), where test_case_is_sound changes its border pixel)
# 16-bit stores of the chain families that neither a `big` nor a `sub` case can cover inside the budget: (family, type, planes or None,
# regime) -> (stores, the measured budget)
NOT_EXERCISED_EDGE = {}


def edge_builders(plain):
    """-> {case id: builder} of the edge cases: shapes of `plain` (builders()) under the name <existing name>_<regime>"""
    out = {}
    for family, rows in EDGE_SINGLES.items():
        for name, codes in rows:
            for regime, dt in [(r, dt) for code, r in (('B', 'big'), ('w', 'subw'), ('x', 'subx')) if code in codes for dt in ((H16, BF) if r == 'big' else (H16,))]:
                assert f'{family}/{name}/{IDS[dt]}' in plain
                out[f'{family}/{name}_{regime}/{IDS[dt]}'] = lambda family=family, name=name, regime=regime, dt=dt: _edge_single(family, name, regime, dt)
    out[f'mac/{_mac_name()}_big/bf16'] = lambda: single('mac', _mac_name() + '_big', BF, *EDGE_MAC, 3, 1, 1, regime='big')
    vname = '{}x{}x{}_big'.format(*EDGE_VGG_STEM)
    out[f'vgg_stem/{vname}/bf16'] = lambda: vgg_stem_case(*EDGE_VGG_STEM, name=vname, powers=VGG_STEM_BIG, regime='big')
    for (planes, regime, dt), (xg, xpow, powers) in EDGE_CHAINS['gauss_tail'].items():
        n, h, w = EDGE_TAIL
        name = f'{n}x{h}x{w}_{regime}'
        out[f'gauss_tail/{name}/{IDS[dt]}'] = lambda name=name, regime=regime, dt=dt, xg=xg, xpow=xpow, powers=powers: chain(
            'gauss_tail', name, dt, EDGE_TAIL[0], 16, *EDGE_TAIL[1:], tail_specs(), xgrid=xg, first=RECIPE[H16], covers=(0,), xpow=xpow, powers=powers, regime=regime, salt=EDGE_TAIL_SALT[regime, dt])
    for (planes, regime, dt), (xg, xpow, powers) in EDGE_CHAINS['gauss_subnet'].items():
        n, h, w = EDGE_SUBNET
        name = f'{n}x{h}x{w}_act1_{regime}'
        out[f'gauss_subnet/{name}/{IDS[dt]}'] = lambda name=name, regime=regime, dt=dt, xg=xg, xpow=xpow, powers=powers: chain(
            'gauss_subnet', name, dt, EDGE_SUBNET[0], 64, *EDGE_SUBNET[1:], subnet_specs(1), xgrid=xg, covers=(0, 1, 2, 3), xpow=xpow, powers=powers, regime=regime)
    for (n, cin, p, h, w, sep) in EDGE_BNECK:
        for (planes, regime, dt), (xg, xpow, powers) in EDGE_CHAINS['bneck'].items():
            if planes != p:
                continue
            name = f'{cin}-{p}x{h}x{w}' + ('_sep' if sep else '') + f'_{regime}'
            out[f'bneck/{name}/{IDS[dt]}'] = lambda name=name, a=(n, cin, h, w), p=p, sep=sep, regime=regime, dt=dt, xg=xg, xpow=xpow, powers=powers: chain(
                'bneck', name, dt, *a, bneck_specs(p), keep=1, res_last='sep' if sep else 'x', xgrid=xg, covers=(0, 1, 2), xpow=xpow, powers=powers, regime=regime)
    return out


def _mac_name():
    n, cin, h, w, cout = EDGE_MAC
    return f'{cin}x{h}x{w}-{cout}'


def _edge_single(family, name, regime, dt):
    """the single-layer case family/name of builders() in an edge regime, under the name <name>_<regime>"""
    new = f'{name}_{regime}'
    if family == 'igemm':
        c = IGEMM[name]
        return single(family, new, dt, *c[:8], regime=regime, **_opts(c[8]))
    if family == 'dma':
        c = DMA[name]
        return single(family, new, dt, *c[:8], keep=1, regime=regime, **_opts(c[8]))
    if family == 'splitk':
        (n, cin, h, w, cout, k, stride, act) = SPLITK[0]
        return single(family, new, dt, n, cin, h, w, cout, k, stride, k // 2, act=act, res='same' if name.endswith('_res') else None, keep=1, regime=regime)
    if family == 'conv1x1':
        (n, cin, h, w, cout, stride, res, act), = [c for c in C1X1 if f'{c[1]}x{c[2]}x{c[3]}-{c[4]}s{c[5]}{c[6]}' == name]
        return single(family, new, dt, n, cin, h, w, cout, 1, stride, 0, act=act, res=res or None, regime=regime)
    if family == 'halo':
        (n, cin, h, w, cout, pool), = [c for c in HALO if f'{c[1]}x{c[2]}x{c[3]}-{c[4]}' + ('_pool' if c[5] else '') == name]
        return single(family, new, dt, n, cin, h, w, cout, 3, 1, 1, pool=pool, regime=regime)
    if family == 'atlas':
        return single(family, new, dt, 3, 128, 21, 30, 256, 3, 1, 1, regime=regime)
    if family == 'thin_out':
        (cout, cin, h, w), = [c for c in THIN_OUT if f'{c[1]}x{c[2]}x{c[3]}-{c[0]}' == name]
        return single(family, new, dt, 2, cin, h, w, cout, 3, 1, 1, act=0, f32=True, regime=regime)
    if family == 'thin3x3':
        (n, h, w, cout, up), act = [c for c in THIN3X3 if name.startswith(f'{c[0]}x{c[1]}x{c[2]}-{c[3]}' + ('_up' if c[4] else '') + '_act')][0], int(name[-1])
        return single(family, new, dt, n, 64 if up else 32, h, w, cout, 3, 1, 1, act=act, in_up=up, regime=regime)
    assert family == 'gln_stem'
    n, h, w = (int(v) for v in name.split('x'))
    return gln_stem_case(dt, n, h, w, regime)


# the work-list launches of test_gpu_exact.py test_list_and_strip_launches: the S = 64 construction of tests/test_gpu_footprint.py
WL_S, WL_N, WL_EXT, WL_POOL_MASK = 64, 4, [[30, 64], [4, 64], [20, 0]], 0b0100100
WL_LAYERS = [[32, 32, 8, 8, 3, 64, 64, 0, 1], [32, 32, 16, 32, 4, 32, 32, 3, 2], [16, 16, 8, 8, 6, 32, 32, 4, 3], [16, 16, 16, 16, 7, 16, 16, 6, 3]]   # `cvpce_skip_layer` fields
WL_CONVS = {1: (64, 128, 32, False), 2: (128, 256, 32, True), 3: (256, 264, 16, False)}      # layer -> cin, cout, input size, fused pool


@lru_cache(maxsize=None)
def worklist_model():
    import footprint                 # tests/footprint.py
    return footprint.worklist_model(WL_EXT + [[WL_S, WL_S]], WL_S, WL_POOL_MASK, WL_LAYERS)


def worklist_case(li):
    """The operands of work-list layer li AS THE REFERENCE SEES THEM: image n - 1 is the constant crop, and a crop's own values end at its
    content extent (the stem: WL_EXT; a conv layer: the input extent its list entries carry in bits 32..55, rows << 12 | columns) --
    beyond it the tensor holds the constant crop's pixels, which is what a list launch reads there.  Layer 0 is the fused stem (its
    constant crop is one grid value per channel); every conv layer has exact operands of its own on the coarse recipe: five layers deep,
    a chain would leave the budget."""
    if li == 0:
        c = vgg_stem_case(WL_N, WL_S, WL_S, name='stem')
        c.x[-1] = c.x[-1, :, :1, :1]
        inside = torch.zeros(WL_N, 1, WL_S, WL_S, dtype=torch.bool)
        for i, (ey, ex) in enumerate(WL_EXT):
            inside[i, :, :ey, :ex] = True
    else:
        cin, cout, hin, pool = WL_CONVS[li]
        c = single('worklist', f'layer{li}', BF, WL_N, cin, hin, hin, cout, 3, 1, 1, pool=pool)
        inside = torch.zeros(WL_N, 1, hin, hin, dtype=torch.bool)
        want, swant, _, _ = worklist_model()[li]
        for en in want + swant:
            inside[(en >> 16) & 0xFFFF, :, :(en >> 44) & 0xFFF, :(en >> 32) & 0xFFF] = True
    inside[-1] = True
    c.x = torch.where(inside, c.x, c.x[-1:])
    c.family, c.id = 'worklist', f'worklist/{c.name}/bf16'
    return c


def _add_worklist(out):
    out['worklist/stem/bf16'] = lambda: worklist_case(0)
    for li in WL_CONVS:
        out[f'worklist/layer{li}/bf16'] = lambda li=li: worklist_case(li)
    return out


BUILDERS = _add_worklist(builders())
EDGE_IDS = []                        # the ids of the edge cases, in the order of IDS_ALL


def _add_edges(out):
    edges = edge_builders(out)
    assert all(cid.rsplit('_', 1)[0] + cid[cid.rindex('/'):] in out for cid in edges), 'an edge case is named after an existing case'
    EDGE_IDS.extend(edges)
    out.update(edges)
    return out


BUILDERS = _add_edges(BUILDERS)
IDS_ALL = list(BUILDERS)


@lru_cache(maxsize=8)
def case(cid):
    return BUILDERS[cid]()


def ids(family, dt=None):
    return [c for c in IDS_ALL if c.startswith(family + '/') and (dt is None or c.endswith('/' + IDS[dt]))]
