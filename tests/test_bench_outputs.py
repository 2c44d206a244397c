"""bench.py's plain line and --dump-outputs on the GPU: the plain run carries the headline only, the dump holds what the last
timed step computed (its IQ is the OFDM modulation of its grids, checked against the CPU oracle; for the wire format the
int16 samples and the amplitude controller's measurements too), and two runs with the same arguments dump the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import backends
import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--slots", "16",
           "--dump-outputs", str(out_dir)] + list(extra)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["config3", "config4", "wire"])
def test_bench_plain_line_and_dumped_outputs(tmp_path, leg):
    extra = {"config3": [], "config4": ["--config", "4"], "wire": ["--wire"]}[leg]
    out = _bench(tmp_path / "a", *extra)
    assert out["metric"] == "pdsch_slots_per_sec" and out["unit"] == "slots/s" and out["higher_is_better"] is True
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"]
    for moved in ("secondary", "cpu_baseline", "verified_vs_oracle"):
        assert moved not in out, moved
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grid.npy", "iq.npy"] + (["iq_stats.npy"] if leg == "wire" else []) + ["slots.npy"], names
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    slots = got["slots"].astype(np.int64)
    assert len(slots) == 8 and np.all(np.diff(slots) > 0) and slots.min() >= 0 and slots.max() < 16
    _, nof_ports, nof_subc, ofdm = cases.baseline_config(3)   # (config 4's cells use the same grid and modulator)
    assert got["grid"].shape == (8, nof_ports, 14, nof_subc, 2)
    assert got["iq"].shape[:2] == (8, nof_ports) and got["iq"].shape[3] == 2
    o = backends.oracle()
    lib = backends.pkg.lib
    abi = backends.abi
    # bench.py's wire-format setting: the amplitude controller as the reference's radio unit sets it
    amplitude = abi.AmplitudeCfg(0, 1, -(10.0 * float(np.log10(nof_subc)) + 12.0), 1.0, -0.1)
    for k, s in enumerate(slots):
        grid = (got["grid"][k].view(np.uint32) >> 16).astype(np.uint16)
        assert np.any(grid)
        # slot i of the batch sits at slot i % 2 of its subframe
        want = o.ofdm_slot(ofdm, grid, int(s) % 2)
        size = lib.slot_size(ofdm, int(s) % 2)
        assert want.shape[1] == size
        if leg != "wire":
            # the dumped IQ is the modulation of the dumped grid
            iq = got["iq"][k].view(np.complex64)[..., 0][:, :size]
            assert float(np.abs(iq - want).max() / np.abs(want).max()) < 1e-5, s
            continue
        for p in range(nof_ports):
            # int16 samples (one LSB: the two FFTs differ by 1e-7 relative) and the measurements of each buffer
            y, m = o.amplitude_control(amplitude, want[p])
            w16 = o.iq_convert_ci16(y, 32767.0).reshape(-1, 2)
            assert np.abs(got["iq"][k, p, :size] - w16).max() <= 1, (s, p)
            sum_power, peak_power, nof_clipped, nof_samples = got["iq_stats"][k, p]
            assert nof_samples == size and abs(nof_clipped - m["nof_clipped"]) <= 2, (s, p, nof_clipped, m["nof_clipped"])
            assert abs(peak_power - m["stats"].peak_power) <= 1e-4 * m["stats"].peak_power, (s, p, peak_power)
            assert abs(sum_power - m["stats"].sum_power) <= 1e-4 * m["stats"].sum_power, (s, p, sum_power)
    if leg == "config3":
        # same arguments, same inputs: the same outputs
        _bench(tmp_path / "b", *extra)
        for n in names:
            assert np.array_equal(np.load(tmp_path / "b" / n), got[n[:-4]]), n
