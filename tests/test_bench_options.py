"""bench.py's plain run and its two options: `--dump-outputs DIR` (the log-posteriors of the last timed step as .npy, the same from
run to run) and `--full` (everything beside the headline).  The helper on the CPU; the runs themselves on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_npy_and_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    a64 = np.linspace(-3.0, 7.0, 1000)
    a32 = np.arange(12, dtype=np.float32).reshape(3, 4)
    ai = np.arange(5)
    bench.dump_outputs(str(tmp_path / 'a'), {'logp': a64, 'single': a32, 'counts': ai})
    got = {n: np.load(str(tmp_path / 'a' / (n + '.npy'))) for n in ('logp', 'single', 'counts')}
    assert got['logp'].dtype == np.float64 and np.array_equal(got['logp'], a64)
    assert got['single'].dtype == np.float32 and np.array_equal(got['single'], a32)
    assert got['counts'].dtype == np.float64 and np.array_equal(got['counts'], ai)      # float32 or float64, nothing else
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    # over the limit: a fixed sample of the elements, in index order, within the limit, identical from call to call
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 2 * 800)
    big = {'x': a64, 'y': a64[::-1].copy()}
    bench.dump_outputs(str(tmp_path / 'b'), big)
    bench.dump_outputs(str(tmp_path / 'c'), big)
    total = 0
    for n in ('x', 'y'):
        b, c = np.load(str(tmp_path / 'b' / (n + '.npy'))), np.load(str(tmp_path / 'c' / (n + '.npy')))
        assert np.array_equal(b, c) and b.size == 100 and np.isin(b, a64).all()
        total += b.nbytes
    assert total <= 2 * 800
    assert np.all(np.diff(np.load(str(tmp_path / 'b' / 'x.npy'))) > 0)                    # index order of an increasing array


def _plain_run(tmp_path, tag, steps):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1                                                                # ONE line
    return json.loads(lines[0]), np.load(str(out / 'logp.npy'))


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_the_same_outputs_every_time(tmp_path):
    """A plain run: one timed region of exactly `--steps` steps, the contract's fields, none of the side measurements; the dumped
    log-posteriors are finite float64, one per walker, and bit-identical between two runs whatever the number of steps."""
    d3, a = _plain_run(tmp_path, 'a', 3)
    d5, b = _plain_run(tmp_path, 'b', 5)
    for d, n in ((d3, 3), (d5, 5)):
        assert d['metric'] == 'walker-likelihoods/sec at 512^2 map, 500-pt grid' and d['unit'] == 'walker-likelihoods/s'
        assert d['higher_is_better'] is True and d['dtype'] == 'f64' and d['n_gpus'] == 1 and d['full'] is False
        assert d['steps'] == n and d['warmup'] == 1 and d['timed_regions'] == 1
        assert d['ms_per_step'] > 0 and abs(d['timed_ms_total'] - n * d['ms_per_step']) <= 1e-9 * d['timed_ms_total']
        assert abs(d['value'] - d['config']['walkers_per_gpu'] / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
        for k in ('cpu_baseline', 'roofline', 'north_star_route', 'host_pointer', 'fp32_variant', 'other_configs', 'parity_max_rel_err'):
            assert k not in d, k
    assert a.dtype == np.float64 and a.shape == (1024,) and np.isfinite(a).all()
    assert np.array_equal(a, b)
