"""Exact k-nearest-neighbour search for k above 16 (csrc/match.hip, the large-k path: distance block -> per-query radix select ->
LDS bitonic sort -> merge passes): same contract as the fused k <= 16 path -- the k smallest (distance, row) pairs in lexicographic
order, NaN distances as +inf, distances bit-identical to the fused path's -- for every k up to the gallery size."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float32]
# Against the fp32 CPU oracle: at 1 600 x 10 000 x 1 024 with f32 rows the two fp32 dot products (matrix pipe, CPU BLAS) differ by up to
# 2.2e-6 over the whole distance matrix (bf16 rows: 0.9e-6), so ranks are compared where neighbours lie more than twice that apart,
# and distances to a little above it.  (Against the matcher's OWN distances the ranking is exact: the prefix tests below.)
SEP, ATOL = 5e-6, 3e-6


def _operands(qn, gn, d, seed, specials=False):
    g = torch.Generator().manual_seed(seed)
    G = F.normalize(torch.rand(gn, d, generator=g), dim=1)     # non-negative like MAC descriptors
    Q = F.normalize(torch.rand(qn, d, generator=g), dim=1)
    if specials:
        G[gn // 2] = G[3]                                      # duplicate rows: a tie for every query
        G[gn - 1] = G[0]
        Q[1, 5] = float('nan')                                 # a NaN query: every distance +inf -> rows 0, 1, 2, ...
    return Q, G


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('qn,gn,d', [(200, 10000, 512), (37, 3200, 1024), (333, 1357, 256), (1600, 10000, 1024)])
def test_large_k_prefix_equals_fused_top16(cuda, dtype, qn, gn, d):
    from cvpce_amd import ops
    Q, G = _operands(qn, gn, d, qn * 7 + gn, specials=True)
    Qd, Gd = Q.to(dtype).to(cuda), G.to(dtype).to(cuda)
    i16, d16 = ops.match_topk(Qd, Gd, 16, return_distance=True)
    i_all, d_all = ops.match_topk(Qd, Gd, gn, return_distance=True)
    for k in (17, 100, gn):
        idx, dist = ops.match_topk(Qd, Gd, k, return_distance=True)
        assert idx.shape == (qn, k) and dist.shape == (qn, k) and idx.dtype == torch.int64 and dist.dtype == torch.float32
        assert idx[:, :16].equal(i16), k
        assert _bits(dist[:, :16]).equal(_bits(d16)), k
        assert idx.equal(i_all[:, :k]) and _bits(dist).equal(_bits(d_all[:, :k])), k      # every k: a prefix of the full ranking
        assert idx[1].cpu().equal(torch.arange(k)), k          # the NaN query
        assert bool(torch.isinf(dist[1]).all())
        assert int(idx.min()) >= 0 and int(idx.max()) < gn


def test_large_k_prefix_on_128_query_tiles(cuda):
    """768 x 10 000: whole rounds of the chip favour the 128-row core's 128-query tiles (474 tiles in one round of 512 slots), bf16
    instances no other shape of this file reaches.  With that core pinned: k = 17 (the storing instance) against k = 16 (the selecting one)."""
    import ctypes
    from cvpce_amd import ops
    from cvpce_amd._lib import lib
    qn, gn, d = 768, 10000, 64
    Q, G = _operands(qn, gn, d, qn * 7 + gn, specials=True)
    Qd, Gd = Q.to(torch.bfloat16).to(cuda), G.to(torch.bfloat16).to(cuda)
    try:
        assert ops.match_set_core(1, 0, 0) == 0
        for k, path in ((16, 0), (17, 2)):
            out = (ctypes.c_longlong * 12)()
            assert lib.cvpce_match_plan(qn, gn, d, k, 0, out) == 0
            assert (out[0], out[1]) == (path, 128)              # path, queries per tile
        i16, d16 = ops.match_topk(Qd, Gd, 16, return_distance=True)
        i17, d17 = ops.match_topk(Qd, Gd, 17, return_distance=True)
    finally:
        ops.match_set_core(0, 0, 0)
    assert i17[:, :16].equal(i16) and _bits(d17[:, :16]).equal(_bits(d16))
    assert i17[1].cpu().equal(torch.arange(17)) and bool(torch.isinf(d17[1]).all())      # the NaN query
    assert int(i17.min()) >= 0 and int(i17.max()) < gn
    assert bool((d17[:, 16] >= d17[:, 15]).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('qn,gn,d', [(200, 10000, 512), (1600, 10000, 1024)])
def test_large_k_oracle_parity(cuda, dtype, qn, gn, d):
    from cvpce_amd import ops
    from oracle import match as omatch
    Q, G = _operands(qn, gn, d, qn + gn)
    Gd, Qd = G.to(dtype), Q.to(dtype)
    ref_d = omatch.cosine_distance_matrix(Gd.float(), Qd.float())    # oracle on the same (rounded) operands
    srt = torch.sort(ref_d, dim=-1, stable=True)
    for k in (17, 100, 1000):
        idx, dist = ops.match_topk(Qd.to(cuda), Gd.to(cuda), k, return_distance=True)
        idx, dist = idx.cpu(), dist.cpu()
        # index-exact at every position whose oracle distance is more than SEP from both neighbours in the ranking (whole rows
        # free of near-ties over 1 000 neighbours are too rare at 10 000 gallery rows to be the mask)
        gap = (srt.values[:, 1:k + 1] - srt.values[:, :k]) > SEP
        sep = gap.clone()
        sep[:, 1:] &= gap[:, :-1]
        assert sep.float().mean() > 0.3, k
        assert idx[sep].equal(srt.indices[:, :k][sep]), k
        if k == 17:                                            # whole rows, as in test_match_parity
            safe = gap.all(dim=1)
            assert safe.float().mean() > 0.1
            assert idx[safe].equal(srt.indices[safe, :k])
        torch.testing.assert_close(dist, ref_d.gather(1, idx), rtol=0, atol=ATOL)


@pytest.mark.parametrize('dtype', DTYPES)
def test_full_ranking(cuda, dtype):
    from cvpce_amd import ops
    qn, gn, d = 50, 1357, 256
    Q, G = _operands(qn, gn, d, 11, specials=True)
    idx, dist = ops.match_topk(Q.to(dtype).to(cuda), G.to(dtype).to(cuda), gn, return_distance=True)
    idx, dist = idx.cpu(), dist.cpu()
    assert idx.sort(dim=1).values.equal(torch.arange(gn).expand(qn, gn))
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    # equal distances: ascending rows
    tie = dist[:, 1:] == dist[:, :-1]
    assert bool((idx[:, 1:][tie] > idx[:, :-1][tie]).all())
    # an all-identical gallery: every distance ties, the ranking is the row order
    Gs = G[:1].expand(gn, d).contiguous()
    idx = ops.match_topk(Q.to(dtype).to(cuda), Gs.to(dtype).to(cuda), gn).cpu()
    assert idx.equal(torch.arange(gn).expand(qn, gn))


@pytest.mark.parametrize('dtype', DTYPES)
def test_beyond_one_lds_sort_run(cuda, dtype):
    """k above 16 384: sorted runs merged through the workspace."""
    from cvpce_amd import ops
    from oracle import match as omatch
    qn, gn, d = 3, 40000, 64
    Q, G = _operands(qn, gn, d, 40000, specials=True)
    G[7] = G[30000]                                            # a tie across two sort runs
    Qd, Gd = Q.to(dtype), G.to(dtype)
    ref_d = omatch.cosine_distance_matrix(Gd.float(), Qd.float())
    i16, d16 = ops.match_topk(Qd.to(cuda), Gd.to(cuda), 16, return_distance=True)
    for k in (20000, gn):
        idx, dist = ops.match_topk(Qd.to(cuda), Gd.to(cuda), k, return_distance=True)
        assert idx[:, :16].equal(i16) and _bits(dist[:, :16]).equal(_bits(d16))
        idx, dist = idx.cpu(), dist.cpu()
        assert idx[1].equal(torch.arange(k))                    # the NaN query
        for q in (0, 2):
            assert idx[q].unique().numel() == k
            assert bool((dist[q, 1:] >= dist[q, :-1]).all())
            tie = dist[q, 1:] == dist[q, :-1]
            assert bool((idx[q, 1:][tie] > idx[q, :-1][tie]).all())
            torch.testing.assert_close(dist[q], ref_d[q].gather(0, idx[q]), rtol=0, atol=ATOL)
            # index-exact against the oracle's stable order where neighbouring distances are apart
            srt = torch.sort(ref_d[q], stable=True)
            sep = torch.ones(gn, dtype=torch.bool)
            gap = (srt.values[1:] - srt.values[:-1]) > SEP
            sep[1:] &= gap
            sep[:-1] &= gap
            sep = sep[:k]
            assert int(sep.sum()) > 1000
            assert idx[q][sep].equal(srt.indices[:k][sep])
        if k == gn:
            assert idx.sort(dim=1).values.equal(torch.arange(gn).expand(qn, gn))


@pytest.mark.parametrize('dtype', DTYPES)
def test_chunked_batch_equals_single_queries(cuda, dtype):
    """1 500 queries against 100 000 rows do not fit one chunk of the workspace budget: every row of the batched result must equal
    the same query searched alone."""
    from cvpce_amd import ops
    from cvpce_amd._lib import lib
    qn, gn, d, k = 1500, 100000, 64, 17
    assert lib.cvpce_match_workspace_bytes(qn, gn, k) < qn * gn * 4        # several chunks
    Q, G = _operands(qn, gn, d, 99, specials=True)
    Qd, Gd = Q.to(dtype).to(cuda), G.to(dtype).to(cuda)
    idx, dist = ops.match_topk(Qd, Gd, k, return_distance=True)
    for q in list(range(0, 8)) + [639, 640, 641, 1279, 1280, 1281, 1499]:
        i1, d1 = ops.match_topk(Qd[q:q + 1].contiguous(), Gd, k, return_distance=True)
        assert idx[q:q + 1].equal(i1), q
        assert _bits(dist[q:q + 1]).equal(_bits(d1)), q


def test_public_surface(cuda):
    from cvpce_amd import classification_eval, production, synthetic
    from cvpce_amd.models.classification import nearest_neighbors
    from oracle import match as omatch
    # nearest_neighbors (classification.py:90-95)
    Q, G = _operands(64, 3000, 128, 5)
    nn = nearest_neighbors(G.to(cuda), Q.to(cuda), k=50)
    assert nn.shape == (64, 50)
    ref_d = omatch.cosine_distance_matrix(G, Q)
    torch.testing.assert_close(ref_d.gather(1, nn.cpu()), ref_d.sort(dim=1).values[:, :50], rtol=0, atol=2e-6)

    # Classifier with k = 20: 20 labels per crop, the first one the k = 1 classifier's
    enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
    gal = synthetic.gallery_images(24, seed=100)
    c1 = production.Classifier(enc, synthetic.TensorGallery(gal), device=cuda, emb_device=cuda, batch_size=8)
    c20 = production.Classifier.from_embedding(enc, c1.embedding, c1.annotations, device=cuda, emb_device=cuda, k=20)
    crops = ((gal[:10] + 1) / 2).clamp(0, 1)
    r1, r20 = c1.classify(crops), c20.classify(crops)
    assert len(r20) == 10 and all(len(r) == 20 for r in r20)
    assert [r[0] for r in r20] == [r[0] for r in r1]
    assert all(len(set(r)) == 20 for r in r20)

    # eval_dihe with k = (1, 5, 20): accuracies non-decreasing in k
    testset = []
    for j in range(4):
        picks = [(j * 5 + t) % 24 for t in range(5)]
        shelf = torch.full((3, 300, 5 * 270), 0.3)
        boxes, targets = [], []
        for t, i in enumerate(picks):
            x = 10 + t * 270
            shelf[:, 20:276, x:x + 256] = ((gal[i] + 1) / 2).clamp(0, 1) * 0.9 + 0.05
            boxes.append([x + 8, 28, x + 240, 260])
            targets.append(c1.annotations[i])
        testset.append((shelf, targets, torch.tensor(boxes)))
    acc = classification_eval.eval_dihe(enc, synthetic.TensorGallery(gal), testset, 8, k=(1, 5, 20))
    assert set(acc) == {1, 5, 20}
    assert acc[1] <= acc[5] <= acc[20] and acc[20] > 0


def test_cli_dihe_eval_knn_20(cuda, tmp_path):
    """`dihe eval --knn 1 --knn 20` in a fresh process: the reference's CLI with a k above the fused path's limit."""
    from PIL import Image
    from cvpce_amd import synthetic
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    enc = synthetic.synthetic_macvgg(seed=1)
    torch.save({'model_state_dict': enc.state_dict()}, tmp_path / 'dihe.tar')
    gal = (synthetic.gallery_images(24, seed=5) + 1) / 2
    names = []
    for i in range(24):
        dd = tmp_path / 'Training' / 'Food' / f'Cat{i % 3}'
        dd.mkdir(parents=True, exist_ok=True)
        to_img(gal[i]).save(dd / f'{10 + i}.png')
        names.append(f'Food/Cat{i % 3}/{10 + i}')
    (tmp_path / 'Testing' / 'store1' / 'images').mkdir(parents=True)
    (tmp_path / 'ann').mkdir()
    for img_id, picks in ((15, (3, 1, 4)), (16, (0, 5, 22))):
        shelf = torch.full((3, 300, 840), 0.3)
        rows = []
        for j, i in enumerate(picks):
            x = 10 + j * 270
            shelf[:, 20:276, x:x + 256] = gal[i]
            rows.append(f'{names[i]}.jpg, {x}, 20, {x + 256}, 276')
        to_img(shelf).save(tmp_path / 'Testing' / 'store1' / 'images' / f'store1_{img_id}.jpg', format='PNG')
        (tmp_path / 'ann' / f's1_{img_id}.csv').write_text('\n'.join(rows) + '\n')
    cmd = [sys.executable, '-m', 'cvpce_amd.cli', 'dihe', 'eval', '--img-dir', str(tmp_path / 'Training'), '--test-imgs',
           str(tmp_path / 'Testing'), '--annotations', str(tmp_path / 'ann'), '--enc-weights', str(tmp_path / 'dihe.tar'),
           '--knn', '1', '--knn', '20']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('--> accuracy')][-1]
    acc = eval(line.split('--> accuracy ', 1)[1])
    assert acc == {1: 1.0, 20: 1.0}          # exact 256 x 256 pastes of gallery products: every crop is its own product
