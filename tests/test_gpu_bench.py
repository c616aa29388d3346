"""bench.py's command line on the GPU at a small size: a plain run times its steps and stops, a
--full run goes on to the checks and the other legs, and --dump-outputs writes the same seeded
sample of the last step's planes in both."""
import json
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
PIXELS = 300_001  # odd, more than the DUMP_PIXELS a dump holds


def _run(monkeypatch, capsys, *args):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--pixels', str(PIXELS)]
                        + list(args))
    for v in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(v, raising=False)
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_is_lean_and_full_run_checks(tmp_path, monkeypatch, capsys):
    plain = _run(monkeypatch, capsys, '--steps', '3', '--warmup', '1',
                 '--dump-outputs', str(tmp_path / 'plain'))
    assert plain['full'] is False and plain['steps'] == 3 and plain['warmup'] == 1
    assert plain['ms_per_step'] > 0 and plain['unit'] == 'Mpixels/s' and plain['dtype'] == 'f64'
    assert plain['higher_is_better'] is True
    # value and ms_per_step describe the same timed steps (ms_per_step is rounded to 1e-3 ms,
    # value to 1e-4 Mpx/s)
    ms = plain['ms_per_step']
    assert plain['value'] == pytest.approx(PIXELS / ms / 1e3, rel=0.00051 / ms, abs=1e-4)
    assert plain['jit']['tiles_jit_timed'] == 3 and plain['jit']['tiles_fallback_timed'] == 0
    for k in ('parity_sample', 'status_numeric_pixels', 'joined_steps', 'end_to_end',
              'n_gt_1_tiling', 'exchange_check'):
        assert plain[k] is None, k
    assert plain['load_stage']['alone'] is None and 'cpu_baseline' not in plain

    full = _run(monkeypatch, capsys, '--steps', '2', '--warmup', '1', '--full',
                '--cpu-seconds', '0.2', '--dump-outputs', str(tmp_path / 'full'))
    assert full['full'] is True and full['steps'] == 2
    assert full['parity_sample']['pixels'] == 16384
    assert full['parity_sample']['mismatched_values'] == 0
    assert full['status_numeric_pixels'] == 0
    assert full['joined_steps']['value'] > 0 and full['end_to_end']['value'] > 0
    assert full['load_stage']['alone']['ms'] > 0 and full['cpu_baseline']['value'] > 0

    # the dumps: the same seeded pixels of every plane, binary64, whatever else the run did
    assert plain['dumped_outputs'] == full['dumped_outputs']
    assert set(plain['dumped_outputs']) == {'status', 'matched', 'class_val', 'onset_year',
                                            'duration', 'magnitude'}
    n_rules = len(bench.CONFIGS['c2']['rules'])
    for f, shape in plain['dumped_outputs'].items():
        a = np.load(tmp_path / 'plain' / (f + '.npy'))
        b = np.load(tmp_path / 'full' / (f + '.npy'))
        assert a.dtype == np.float64 and list(a.shape) == shape
        assert shape == ([bench.DUMP_PIXELS] if f == 'status' else [n_rules, bench.DUMP_PIXELS])
        assert np.array_equal(a, b, equal_nan=True), f
    m = np.load(tmp_path / 'plain' / 'matched.npy')
    assert set(np.unique(m)) <= {0.0, 1.0} and m.any()
