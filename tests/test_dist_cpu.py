"""The N>1 path rehearsed with world_size-2 (and 3) gloo processes on the CPU:
image sharding is a partition, the sharded gallery build + one all_gather reproduces the single-rank
gallery bit-for-bit, max-over-ranks timing reduction works."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _fake_embed(x):
    """Deterministic stand-in for the GPU embedder in this host-logic test: (b,3,8,8) -> (b,6)."""
    return torch.stack([x.mean(dim=(1, 2, 3)), x.amax(dim=(1, 2, 3)), x[:, 0].sum(dim=(1, 2)), x[:, 1].sum(dim=(1, 2)),
                        x[:, 2].sum(dim=(1, 2)), x.amin(dim=(1, 2, 3))], dim=1)


def _worker(rank, world, port, n_gallery, n_images, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    from cvpce_amd import dist as cdist
    r, _, w = cdist.init(backend='gloo')
    assert (r, w) == (rank, world)
    gal = torch.rand(n_gallery, 3, 8, 8, generator=torch.Generator().manual_seed(7))
    full = cdist.build_gallery_sharded(_fake_embed, gal, rank, world)
    mine = cdist.shard_images(n_images, rank, world)
    t = cdist.max_over_ranks(float(rank + 1), torch.device('cpu'))
    cdist.barrier()
    # the optional final gather of bench.py --verify: (global image id, digest) pairs from every rank
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, [(g, f'digest-of-{g}') for g in mine])
    merged = {g: d for p in parts for g, d in p}
    q.put((rank, full, mine, t, merged, torch.get_num_threads()))
    dist.destroy_process_group()


def _run_world(world, n_gallery, n_images):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_gallery, n_images, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = [q.get(timeout=240) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return results


@pytest.mark.parametrize('world,n_gallery,n_images', [(2, 11, 16), (2, 4, 3), (3, 10, 64), (8, 3207, 64)])     # the last: BASELINE configs[4]'s
def test_sharded_gallery_and_image_partition(world, n_gallery, n_images):                                       # 8 ranks x 8 images, an uneven gallery (3200 + 7)
    try:
        results = _run_world(world, n_gallery, n_images)
    except Exception:            # a rendezvous port can be taken between _free_port() and bind: one retry
        results = _run_world(world, n_gallery, n_images)
    gal = torch.rand(n_gallery, 3, 8, 8, generator=torch.Generator().manual_seed(7))
    want = _fake_embed(gal)
    seen = []
    for rank, full, mine, t, merged, _ in results:
        assert torch.equal(full, want), f'rank {rank}: gathered gallery differs from the single-rank gallery'
        assert t == float(world)
        assert merged == {g: f'digest-of-{g}' for g in range(n_images)}      # every rank holds every image's digest after the gather
        seen += mine
    assert sorted(seen) == list(range(n_images))        # every image on exactly one rank


def test_shard_range_properties():
    from cvpce_amd import dist as cdist
    for n in (0, 1, 7, 64, 3200):
        for world in (1, 2, 3, 8):
            blocks = [cdist.shard_range(n, r, world) for r in range(world)]
            assert blocks[0][0] == 0 and blocks[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
            sizes = [e - s for s, e in blocks]
            assert max(sizes) - min(sizes) <= 1
    assert cdist.shard_range(64, 3, 8) == (24, 32)       # BASELINE config 5: 8 images per GPU
    assert cdist.all_gather_rows(torch.ones(3, 2), 3, 0, 1).shape == (3, 2)


def test_host_thread_share():
    """bench.py caps every rank's host threads at cores // world (eight ranks on one node each synthesise and stage 403 MB of images
    per step: uncapped they would run 8 x cores OpenMP threads)."""
    import bench
    assert bench.host_threads_for(1, 64) == 64 and bench.host_threads_for(8, 64) == 8 and bench.host_threads_for(8, 4) == 1


def _bench_stub(gpus, extra=()):
    """`python bench.py --gpus N ...` exactly as a user (or the driver's launcher) starts it, with the CPU stand-in pipeline of
    tests/bench_stub.py and the gloo backend: bench.py spawns torch.distributed.run as a child, N ranks run main()."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVPCE_BENCH_STUB='bench_stub:build', CVPCE_DIST_BACKEND='gloo', OMP_NUM_THREADS='1',
               PYTHONPATH=os.pathsep.join([os.path.join(root, 'tests'), root, os.environ.get('PYTHONPATH', '')]))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        det = os.path.join(tmp, 'details.json')
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(gpus), '--steps', '3', '--warmup', '1', '--gallery', '203',
                            '--images-per-gpu', '8', '--verify', '--full', '--allow-stub', '--details', det, *extra], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 prints ONE line, the other ranks nothing
        assert len(lines[0]) < 4096                                   # ... that the driver can parse (round 5's 23 KB line could not be)
        line, full = json.loads(lines[0]), json.load(open(det))
    # a stand-in run is stamped: it can never be mistaken for a measurement
    assert line['stub'] == 'bench_stub:build' and line['metric'].startswith('STUB') and line['data'] == 'stub'
    # the compact line carries what a scaling run is checked by (world size the process group saw, the job digest) without the details file
    assert line['config']['collectives']['world_size'] == full['config']['collectives']['world_size'] == gpus
    assert line['verify'] == {'images': full['verify']['images'], 'digest': full['verify']['digest']}
    assert all(line[k] == full[k] for k in ('value', 'n_gpus', 'steps', 'ms_per_step', 'scaling'))
    return full


def test_bench_main_under_8_gloo_ranks():
    """bench.py main() end to end under 8 ranks (BASELINE configs[4]'s layout: 8 images per rank, 64 in the job) with a CPU stand-in for the
    HIP pipeline: argument parsing, launcher spawn, image sharding, the sharded gallery + ONE all_gather (uneven: 203 rows), three timed
    windows with barriers and MAX-over-ranks, the --verify digest gather, rank 0's side legs not deadlocking the ranks that have none --
    and the per-image digests are the ones a 1-rank and a 2-rank job compute for the same 64 / 16 global images."""
    d8 = _bench_stub(8)
    assert d8['n_gpus'] == 8 and d8['scaling'] == 'weak' and d8['steps'] == 3 and d8['config']['global_images'] == 64
    assert d8['value'] > 0 and abs(d8['value'] - 64 * 3 / (d8['ms_per_step'] * 3e-3)) / d8['value'] < 1e-2       # whole-job images / max-over-ranks time
    assert d8['windows']['n'] == 3
    c = d8['config']['collectives']
    assert c['backend'] == 'gloo' and c['world_size'] == 8 and c['all_gather'] == 1               # the process group saw 8 ranks; ONE gallery all_gather
    assert c['all_gather_bytes_received'] == 8 * 26 * 16 * 4                                       # 8 padded blocks of ceil(203 / 8) = 26 rows x D x f32
    assert c['in_timed_windows'] == {'all_gather': 0, 'all_reduce': 3, 'barrier': 6} and c['data_path_collectives_per_step'] == 0
    v8 = d8['verify']
    assert v8['images'] == 64 and sorted(int(g) for g in v8['per_image']) == list(range(64))
    d2 = _bench_stub(2)
    assert d2['n_gpus'] == 2 and d2['config']['collectives']['world_size'] == 2 and d2['verify']['images'] == 16
    assert all(d2['verify']['per_image'][g] == v8['per_image'][g] for g in d2['verify']['per_image'])     # image g: same result at any world size


def test_bench_dump_outputs_identical_across_runs(tmp_path):
    """`bench.py --dump-outputs DIR` writes what the last timed step returned; with the same arguments two runs write the same arrays
    (the inputs are seeded), so two builds can be compared output for output."""
    import numpy as np
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVPCE_BENCH_STUB='bench_stub:build', OMP_NUM_THREADS='1',
               PYTHONPATH=os.pathsep.join([os.path.join(root, 'tests'), root, os.environ.get('PYTHONPATH', '')]))
    runs = []
    for name in ('a', 'b'):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--gallery', '20',
                            '--images-per-gpu', '4', '--allow-stub', '--details', str(tmp_path / f'{name}.json'), '--dump-outputs', str(d)],
                           capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        full = json.load(open(tmp_path / f'{name}.json'))
        assert full['steps'] == 3 and full['windows']['n'] == 3 and sum(full['windows']['steps_each']) == 3
        runs.append({p.name: np.load(p) for p in d.iterdir()})
        assert set(full['dumped_outputs']) == {n[:-4] for n in runs[-1]}
    assert {'boxes.npy', 'scores.npy', 'indices.npy', 'embeddings.npy', 'counts_host.npy'} <= set(runs[0])
    assert all(a.dtype in (np.float32, np.float64) for a in runs[0].values())
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_gloo_barrier_leaves_the_gpu_alone(monkeypatch, tmp_path):
    """A gloo rank's barrier synchronises on the host: torch's barrier() asks the runtime for the machine's accelerator, which opens
    the GPU in every CPU-only rank of a rehearsal (eight ranks: eight processes holding the device)."""
    import torch.distributed as dist
    from cvpce_amd import dist as cdist

    def no_query():
        raise AssertionError('the gloo barrier queried the accelerator')
    monkeypatch.setattr(torch._C, '_get_accelerator', no_query)
    dist.init_process_group('gloo', init_method=f'file://{tmp_path}/store', rank=0, world_size=1)
    try:
        before = cdist.STATS['barrier']
        cdist.barrier()
        assert cdist.STATS['barrier'] == before + 1
    finally:
        dist.destroy_process_group()
