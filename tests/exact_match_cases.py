"""Operands and float64 reference of the bit-exact matcher tests.  (Not a test module: test_exact_match_cases_cpu.py shows on the host that
every case is sound, test_gpu_match_exact.py runs csrc/match.hip on them and demands equality; the conv kernels' counterpart is
exact_cases.py.)

The tolerance tests feed non-negative unit rows, so every distance lies in a narrow band around 0.25, depends on the fp32 summation
order and can only be compared behind a mask of well-separated neighbours.  Here every row has exactly s non-zero entries, s in
{1, 4, 16, 64, 256}, each +-2^e with one e in [-4, 4] per row:

  * the sum of squares is s 4^e, the norm sqrt(s) 2^e a power of two, its reciprocal exact;
  * all products of one (query, gallery row) pair have the same magnitude 2^(eq + eg), so every partial dot sum in any order is an integer
    multiple of it with a count of at most 256: fp32 adds them without rounding and the summation order drops out;
  * dot / (|q| |g|) is an integer over sqrt(sq sg) <= 256: the distance is a multiple of 2^-8 in [0, 2], formed without rounding both as
    1 - dot / (|q| |g|) (f32 rows) and as fma(-dot, (1 / |q|)(1 / |g|), 1) (bf16 rows);
  * a zero row has its norm clamped to eps, a dot product of 0 and therefore distance exactly 1 in both forms;
  * bf16 holds every entry.

So every distance of the kernel must EQUAL the float64 reference, and with it the whole (distance, row) ranking: no mask, no tolerance.
Distances repeat (a few dozen distinct values per matrix), so ties are everywhere -- at the cut between rank k and k + 1, across the
128-row gallery tiles, across sort runs -- and the tie-break (lower row first) is compared against `torch.sort(stable=True)`.

Two recipes:
  ties    s from {1, 4, 16, 64} (those that fit the width): sparse rows, few distinct distances, ties at every cut.  Planted (as far as
          the case has the rows): a gallery row duplicated into another 128-row tile, a zero gallery row, a zero query, a query that is
          a positive multiple of the duplicated row (distance 0, to both twins), one that is a negative multiple of another row
          (distance 2), a one-hot query.
  dense   s = D for every query, so every feature column enters every dot product of every query: a dropped or doubled K position
          changes every query's distances.  At D = 256 the gallery mixes s in {64, 256}.  Planted: the gallery rows as above and the two
          multiples (a zero or one-hot query would not be dense).
No NaN or Inf operands here: test_gpu_kernels.py and test_gpu_match_large_k.py own those.
"""
import zlib
from functools import lru_cache
from typing import NamedTuple

import torch

EPS = float(torch.tensor(1e-8, dtype=torch.float32))      # the matcher's norm clamp as the kernels hold it: the fp32 value of 1e-8
GRID = 2.0 ** -8                                           # every distance is a multiple of this
TILE_G = 128                                               # gallery rows per tile of the 128-row core (the other core's are 128 or 256)
SORT_RUN = 16384                                           # keys of one LDS sort run of the large-k path
SIZES = (1, 4, 16, 64, 256)
FUSED_KS, LARGE_KS = (1, 4, 16), (17, 100)                 # large-k cases also run k = G


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32('/'.join(str(k) for k in key).encode()))


def recipe_rows(n, d, sizes, g):
    """(n, d) float64: row r has exactly s_r entries +-2^e_r (s_r drawn from `sizes`, e_r from [-4, 4]) at random positions, 0 elsewhere"""
    sizes = torch.tensor([s for s in sizes if s <= d])
    assert len(sizes), (d, sizes)
    s = sizes[torch.randint(0, len(sizes), (n,), generator=g)]
    e = torch.randint(-4, 5, (n,), generator=g)
    place = torch.rand(n, d, generator=g).argsort(dim=1)            # a random permutation per row: the s smallest ranks are the support
    sign = torch.randint(0, 2, (n, d), generator=g).double() * 2 - 1
    return (place < s[:, None]).double() * sign * (2.0 ** e.double())[:, None] + 0.0        # (+ 0.0: no negative zeros)


def _multiple(row, negative):
    """a multiple of a recipe row that stays inside the recipe's scales: x4 | x1/4, or x-1/2 | x-2"""
    top = float(row.abs().max())
    if negative:
        return row * (-0.5 if top >= 2.0 ** -3 else -2.0) + 0.0
    return row * (4.0 if top <= 4.0 else 0.25)


class Reference(NamedTuple):
    q_norms: torch.Tensor      # (Q,) float64, clamped at EPS
    g_norms: torch.Tensor      # (G,)
    dist: torch.Tensor         # (Q, G) float64
    values: torch.Tensor       # (Q, G) float64: every query's distances ascending ...
    indices: torch.Tensor      # (Q, G) int64: ... and their rows, equal distances by ascending row (stable sort)


def reference(Q, G, eps=EPS):
    """float64: norms clamped at eps, dist = 1 - <q, g> / (|q| |g|), the (distance, row) order"""
    Q, G = Q.double(), G.double()
    qn = Q.square().sum(dim=1).sqrt().clamp(min=eps)
    gn = G.square().sum(dim=1).sqrt().clamp(min=eps)
    dist = 1.0 - (Q @ G.T) / (qn[:, None] * gn[None, :])
    srt = torch.sort(dist, dim=1, stable=True)
    return Reference(qn, gn, dist, srt.values, srt.indices)


class MatchCase(NamedTuple):
    name: str
    recipe: str                # 'ties' | 'dense'
    Q: torch.Tensor            # (Q, D) float64
    G: torch.Tensor            # (G, D) float64
    ks: tuple                  # every k the GPU tests search this case with
    planted: dict              # what -> row index (queries: 'q_...', gallery: 'g_...')

    @property
    def shape(self):
        return (self.Q.shape[0], self.G.shape[0], self.Q.shape[1])

    @property
    def ref(self):
        return _reference_of(self.name)


# name -> (recipe, Q, G, D, ks, seed).  The seeds are picked so that test_exact_match_cases_cpu.py's conditions on the inputs hold.
_G_BIG = 16500
SPECS = {
    'ties_1x129x64': ('ties', 1, 129, 64, FUSED_KS, 0),                            # one tile, one query
    'ties_65x129x64': ('ties', 65, 129, 64, FUSED_KS + LARGE_KS + (129,), 0),      # a ragged last tile in both dimensions
    'dense_65x129x64': ('dense', 65, 129, 64, FUSED_KS, 0),
    'ties_130x1000x192': ('ties', 130, 1000, 192, FUSED_KS + LARGE_KS + (1000,), 0),   # several K-steps
    'dense_330x517x256': ('dense', 330, 517, 256, FUSED_KS, 0),                    # more than one 320-query tile
    'ties_768x10000x64': ('ties', 768, 10000, 64, (4, 17), 0),                     # the shape whose bf16 launch takes 128-query tiles
    'ties_3x16500x64': ('ties', 3, _G_BIG, 64, (_G_BIG,), 0),                      # above one LDS sort run
    'ties_33x200x100': ('ties', 33, 200, 100, (3,), 0),                            # a width that pad_features has to fill up
}
FUSED_CASES = ('ties_1x129x64', 'ties_65x129x64', 'dense_65x129x64', 'ties_130x1000x192', 'dense_330x517x256')
LARGE_K_CASES = ('ties_65x129x64', 'ties_130x1000x192')
TQ128_CASE, SORT_RUNS_CASE, PADDED_CASE = 'ties_768x10000x64', 'ties_3x16500x64', 'ties_33x200x100'


@lru_cache(maxsize=None)
def case(name):
    recipe, qn, gn, d, ks, seed = SPECS[name]
    g = seeded('match', name, seed)
    if recipe == 'ties':
        Q, G = recipe_rows(qn, d, SIZES[:4], g), recipe_rows(gn, d, SIZES[:4], g)
    else:
        Q, G = recipe_rows(qn, d, (d,), g), recipe_rows(gn, d, (d,) if d < 256 else (64, 256), g)
        G[3], G[gn // 3] = recipe_rows(2, d, (d,), g)               # the rows the planted queries are multiples of: dense themselves
    planted = {}
    # the twins in different 128-row tiles (and, above one sort run, so far apart that the large-k path sorts them in different runs)
    twin, dup = 3, gn - 1
    assert twin // TILE_G != dup // TILE_G
    G[dup] = G[twin]
    planted['g_twin'], planted['g_duplicate'] = twin, dup
    planted['g_zero'] = gn // 2
    G[gn // 2] = 0
    if qn >= 3:
        planted['q_positive_multiple'], planted['q_negative_multiple'] = 0, qn - 1
        Q[0] = _multiple(G[twin], negative=False)
        Q[qn - 1] = _multiple(G[gn // 3], negative=True)
        planted['g_negated'] = gn // 3
    if recipe == 'ties' and qn >= 6:
        planted['q_zero'], planted['q_one_hot'] = 1, qn - 2
        Q[1] = 0
        Q[qn - 2] = 0
        Q[qn - 2, d // 3] = -0.25
    return MatchCase(name, recipe, Q, G, tuple(ks), planted)


@lru_cache(maxsize=None)
def _reference_of(name):
    c = case(name)
    return reference(c.Q, c.G)


def cut_ties(ref, k):
    """(Q,) bool: the distances at rank k and k + 1 are equal, so which row makes the cut is the tie-break's decision (k < G)"""
    return ref.values[:, k - 1] == ref.values[:, k]


def straddles(ref, k, tile=TILE_G):
    """(Q,) bool: two neighbours of the top k have equal distances and rows in different gallery tiles"""
    v, i = ref.values[:, :k], ref.indices[:, :k]
    return ((v[:, 1:] == v[:, :-1]) & (i[:, 1:] // tile != i[:, :-1] // tile)).any(dim=1)


def select_positions(ref, k):
    """(Q, G) int64: where the large-k path's select puts each gallery row among a query's k survivors, -1 if it is not one: the rows
    below the threshold distance in row order, then the lowest rows at the threshold.  position // SORT_RUN is the LDS sort run."""
    thr = ref.values[:, k - 1:k]
    lt, eq = ref.dist < thr, ref.dist == thr
    nlt = lt.sum(dim=1, keepdim=True)
    pos_lt = lt.cumsum(dim=1) - 1
    pos_eq = nlt + eq.cumsum(dim=1) - 1
    pos = torch.where(lt, pos_lt, torch.where(eq & (pos_eq < k), pos_eq, torch.full_like(pos_lt, -1)))
    return pos


# l2_normalize: (B, D) recipe rows; the quotient by the power-of-two norm is exact, a zero row stays zero
L2_SHAPES = tuple((b, d) for d in (1, 16, 64, 100, 256) for b in (1, 5))


@lru_cache(maxsize=None)
def l2_case(b, d):
    """-> (x (b, d) float64, x / max(|x|, eps) float64); b = 5: row 3 is zero"""
    x = recipe_rows(b, d, SIZES, seeded('l2', b, d))
    if b > 3:
        x[3] = 0
    return x, x / x.square().sum(dim=1, keepdim=True).sqrt().clamp(min=EPS)
