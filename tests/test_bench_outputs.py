"""bench.py's plain run and --dump-outputs: a plain run times the steps and
prints the headline line alone; --full adds the checks and the other figures;
--dump-outputs writes the last timed step's outputs as float32 .npy files, a
fixed seeded sample where an array would take the dump past its share of 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402
from plenum_gpu import synth  # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup')
FULL_ONLY = ('verdict_mismatches', 'roofline', 'kernel_ms', 'cpu_baseline', 'end_to_end', 'small_batch_latency',
             'other_configs')


def test_dump_outputs_is_float32_and_exact_for_small_arrays(tmp_path):
    a = np.arange(1000, dtype=np.uint8).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / 'd'), {'a': a, 'flag': np.array([True, False])})
    got = np.load(tmp_path / 'd' / 'a.npy')
    assert got.dtype == np.float32 and got.shape == a.shape and (got == a).all()
    assert np.load(tmp_path / 'd' / 'flag.npy').tolist() == [1.0, 0.0]


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 2 * 4 * 100)   # 100 float32 elements per array
    big = (np.arange(5000) % 251).astype(np.int32)
    small = np.arange(100, dtype=np.int32)
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small})
    one, two = np.load(tmp_path / 'one' / 'big.npy'), np.load(tmp_path / 'two' / 'big.npy')
    assert one.dtype == np.float32 and one.shape == (100,) and (one == two).all()
    idx = np.sort(np.random.default_rng(0).choice(5000, size=100, replace=False))
    assert (one == big[idx]).all()
    assert (np.load(tmp_path / 'one' / 'small.npy') == small).all()
    total = sum(os.path.getsize(tmp_path / 'one' / f) for f in os.listdir(tmp_path / 'one'))
    assert total <= 2 * 4 * 100 + 2 * 128   # the data + two .npy headers


def test_steps_below_one_is_refused_before_any_gpu_call():
    p = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0'], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and '--steps' in p.stderr and not p.stdout.strip()


def _bench(*argv):
    p = subprocess.run([sys.executable, '-u', os.path.join(REPO, 'bench.py'), '--gpus', '1'] + list(argv), cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:] + p.stdout[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """n = 5000 (no multiple of the bitmap's 64-bit words), 3 timed steps (the
    last one lands in output slot 1 of the pipelined schedule)."""
    n = 5000
    line = _bench('--n', str(n), '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path))
    for k in HEADLINE:
        assert k in line, k
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['unit'] == 'verifies/s' and line['higher_is_better'] is True
    assert abs(line['value'] - n / (line['ms_per_step'] * 1e-3)) <= 1e-3 * line['value']
    assert not [k for k in FULL_ONLY if k in line], line
    assert sorted(os.listdir(tmp_path)) == ['bitmap.npy', 'verdict.npy']
    verdict, bitmap = np.load(tmp_path / 'verdict.npy'), np.load(tmp_path / 'bitmap.npy')
    assert verdict.dtype == np.float32 and bitmap.dtype == np.float32
    want = np.array([not synth.tampered(2, i) for i in range(n)])
    assert verdict.shape == (n,) and (verdict == want).all()
    bits = np.unpackbits(bitmap.astype(np.uint8), bitorder='little')
    assert bits.size == (n + 63) // 64 * 64 and (bits[:n].astype(bool) == want).all() and not bits[n:].any()


@pytest.mark.gpu
def test_full_run_keeps_the_checks_and_the_other_figures():
    line = _bench('--n', '5000', '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline', '--no-e2e')
    for k in HEADLINE:
        assert k in line, k
    assert line['verdict_mismatches'] == 0
    assert line['roofline'] and line['roofline']['frac'] > 0 and line['kernel_ms']['curve'] > 0
    assert line['config']['tampered'] == sum(synth.tampered(2, i) for i in range(5000))
