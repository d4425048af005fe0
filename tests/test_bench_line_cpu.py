"""bench.py's printed line stays under 4 KB whatever the side legs return (round 5's 23 KB line left the round unmeasured: the driver
could not parse it); the full object goes to the details file.  CPU only: no kernels are launched."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _full(bloat):
    """a result object shaped like run_pipeline's, with `bloat` rows in every table that grew in earlier rounds."""
    row = {'launch_class': 'conv_dma_kernel 200x200 128->64 k3 s1', 'launches': 1.0, 'us': 81.8, 'gflop': 23.59, 'mb': 62.0, 'flop_per_byte': 380.3,
           'bound': 'mfma', 'tflops': 288.4, 'frac_of_roof': 0.1154}
    return {
        'metric': 'shelf images/sec end-to-end (detect+embed+match)', 'value': 280.4, 'unit': 'images/s', 'n_gpus': 1, 'steps': 20, 'warmup': 5,
        'ms_per_step': 28.53, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16', 'data': 'synthetic',
        'windows': {'n': 3, 'ms_per_step': [28.5, 28.6, 28.4]},
        'config': {'workload': 'full production path ' + 'x' * 1000, 'images_per_gpu': 8, 'global_images': 8, 'proposals_per_image': 200.0, 'gallery': 3200,
                   'match_dtype': 'bf16', 'detector_precision': 'fp16', 'weights': 'w' * 300, 'parallelism': 'dp1 (images sharded ...)', 'gallery_build_s': 1.0,
                   'collectives': {'backend': 'nccl', 'world_size': 8, 'all_gather': 1, 'all_reduce': 9, 'barrier': 20, 'in_timed_windows': {'a': 1},
                                   'data_path_collectives_per_step': 0}},
        'value_with_h2d': 270.0, 'value_lists_off': 171.0, 'value_planted_boxes': 190.0, 'value_fitted_scenes_p200': 168.0,
        'co_headlines': {'lists_off': {'all_conv_kernels': {f'k{i}': row for i in range(bloat)}}},
        'roofline': {'bound': 'mfma', 'achieved': 1469.7, 'peak': 2500.0, 'unit': 'TFLOP/s', 'frac': 0.5879, 'traffic': 1.133, 'kernel': 'conv3x3_halo2_kernel',
                     'launches': 360, 'avg_launch_us': 1920.0, 'lists_off': {'frac': 0.63, 'avg_launch_us': 1563.9}, 'end_to_end': {'frac_of_mfma_peak': 0.57},
                     'strip_launches': {'launches': 40, 'avg_launch_us': 91.0, 'frac': 0.3, 'total_ms': 3.6},
                     'stages': {k: {'ms_per_step': 1.0, 'note': 'n' * 200} for k in ('detect', 'crop', 'embed', 'match')},
                     'all_conv_kernels': {f'k{i}': row for i in range(bloat)}, 'hbm_stages': {f'k{i}': row for i in range(bloat)},
                     'clocks': {'step': {'sclk_mhz_median': 2050.0, 'power_w_median': 1390.0}}},
        'cpu_baseline': {'value': 0.012, 'unit': 'images/s', 'cores': 16, 'kind': 'port', 'sample': 's' * 600},
        'parity': {'images': 4, 'ap50_vs_oracle': 0.99, 'by_precision': {'fp16': {f'm{i}': 0.1 for i in range(bloat)}}, 'sample': 'p' * 500},
        'workloads': {'detector_configs1': {'images': 4, 'ms_per_step': 2.4, 'images_per_s': 1600.0, 'frac_of_mfma_peak': 0.19, 'layers': {'classes': [row] * bloat}},
                      'match_stress_configs3': [{'P': p, 'G': 10000, 'D': d, 'us_per_launch': 9.9} for p in (200, 1600) for d in (512, 1024)]},
        'verify': {'images': 64, 'digest': 'd' * 64, 'per_image': {str(i): 'h' * 16 for i in range(64)}},
    }


def test_line_is_compact_and_details_complete(tmp_path):
    for bloat in (0, 40, 4000):
        full = _full(bloat)
        path = str(tmp_path / f'details_{bloat}.json')
        s = bench.emit(full, path)
        assert len(s) < 4096 and '\n' not in s
        line = json.loads(s)
        assert all(line[k] == full[k] for k in bench.BASE_KEYS)
        assert line['roofline']['frac'] == 0.5879 and line['roofline']['lists_off_frac'] == 0.63 and line['roofline']['end_to_end_frac'] == 0.57
        assert line['roofline']['strip_launches'] == {'launches': 40, 'avg_launch_us': 91.0, 'frac': 0.3}
        assert line['cpu_baseline']['kind'] == 'port' and len(line['cpu_baseline']['sample']) <= 120
        assert line['config']['collectives'] == {'backend': 'nccl', 'world_size': 8, 'all_gather': 1, 'data_path_collectives_per_step': 0}
        assert line['verify'] == {'images': 64, 'digest': 'd' * 64} and line['details'] == f'details_{bloat}.json'
        assert line['value_lists_off'] == 171.0 and line['value_fitted_scenes_p200'] == 168.0 and line['value_with_h2d'] == 270.0
        assert json.load(open(path)) == json.loads(json.dumps(full))          # nothing is lost: the file holds the whole object


def test_unwritable_details_path_does_not_lose_the_line():
    s = bench.emit(_full(3), '/proc/definitely/not/writable/details.json')
    assert json.loads(s)['details'].startswith('not written')


def test_stub_hook_refused_without_flag():
    """CVPCE_BENCH_STUB alone must not replace the HIP pipeline: bench.py exits with an error and prints no line."""
    env = dict(os.environ, CVPCE_BENCH_STUB='bench_stub:build', PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'tests'), ROOT]))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '1', '--warmup', '0'], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and '--allow-stub' in r.stderr and '{"metric"' not in r.stdout


def test_timed_windows_run_exactly_steps():
    """--steps is the number of timed steps in all: the windows split it, they do not each run it."""
    import torch
    for steps, windows, n_windows in ((10, 3, 3), (2, 3, 2), (1, 3, 1), (7, 1, 1)):
        calls = []
        elapsed, per_step = bench.timed_windows(lambda: calls.append(1), steps, windows, torch.device('cpu'), collective=False)
        assert len(calls) == steps and len(per_step) == n_windows and sum(bench.window_sizes(steps, windows)) == steps
        assert elapsed == sorted(per_step)[len(per_step) // 2] * steps
        st = bench.window_stats(per_step, steps)
        assert st['n'] == n_windows and sum(st['steps_each']) == steps


def test_dump_outputs_types_budget_and_sample(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files (integers exactly, as float64), and a fixed seeded row sample when the
    whole would exceed the budget."""
    import numpy as np
    import torch
    out = {'boxes': torch.arange(24, dtype=torch.float32).view(2, 3, 4), 'emb': torch.ones(5, 2, dtype=torch.bfloat16),
           'indices': torch.tensor([[2 ** 40, -1]]), 'counts_host': [3, 1]}
    shapes = bench.dump_outputs(out, str(tmp_path / 'a'))
    assert shapes == {'boxes': [2, 3, 4], 'emb': [5, 2], 'indices': [1, 2], 'counts_host': [2]}
    got = {k: np.load(tmp_path / 'a' / f'{k}.npy') for k in shapes}
    assert got['boxes'].dtype == np.float32 and got['emb'].dtype == np.float32 and got['indices'].dtype == np.float64
    assert np.array_equal(got['boxes'], out['boxes'].numpy()) and got['indices'][0, 0] == 2 ** 40 and list(got['counts_host']) == [3, 1]
    big = {'x': torch.randn(1000, 64), 'n': torch.arange(4)}
    for d in ('b', 'c'):
        bench.dump_outputs(big, str(tmp_path / d), budget=64 * 1024)
    total = sum(f.stat().st_size for f in (tmp_path / 'b').iterdir())
    assert total <= 64 * 1024 + 4 * 128                               # (+ the .npy headers)
    rows = np.load(tmp_path / 'b' / 'x_rows.npy').astype(np.int64)
    assert np.array_equal(np.load(tmp_path / 'b' / 'x.npy'), big['x'].numpy()[rows]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / 'c' / 'x_rows.npy')) and not (tmp_path / 'b' / 'n_rows.npy').exists()


def test_side_legs_run_only_with_full(monkeypatch):
    """A plain run does only what `value` needs: every side leg's --no-* flag is set unless --full is given; under --full each --no-*
    option still drops its leg.  SIDE_LEG_FLAGS names every --no-* option, so a new leg cannot join plain runs unnoticed."""
    def parsed(*argv):
        monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
        return bench.parse()
    plain = parsed('--gpus', '1', '--steps', '5', '--warmup', '2')
    assert not plain.full and all(getattr(plain, f) for f in bench.SIDE_LEG_FLAGS)
    full = parsed('--gpus', '1', '--steps', '5', '--warmup', '2', '--full')
    assert {k for k in vars(full) if k.startswith('no_')} == set(bench.SIDE_LEG_FLAGS)
    assert not any(getattr(full, f) for f in bench.SIDE_LEG_FLAGS)
    some = parsed('--full', '--no-peaks', '--no-parity')
    assert {f for f in bench.SIDE_LEG_FLAGS if getattr(some, f)} == {'no_peaks', 'no_parity'}
