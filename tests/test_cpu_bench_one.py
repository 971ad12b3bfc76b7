"""bench.py's ``--full`` run at N = 1 on the fake device (the plain run: the last tests here):
besides config 3 (the value) it carries config 2 device-resident, config 5 with the FedOpt hand-out pull timed, and,
because config 4 does not fit one GPU, ONE GPU's share of the 8-GPU split of config 4 labelled as the share (instead of
a skip); the CPU baseline runs after every GPU entry, and every entry records the GPU state it ran at (here: not
available, the fake device has no GPU)."""

import contextlib
import io
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from bench_fake_rank import install, small_presets  # noqa: E402


@pytest.fixture
def undo_install(monkeypatch):
    """install() patches bench, torch.cuda and DeviceContext for the whole process: have monkeypatch put every one back
    after the test (other tests in this process parse bench's real presets)."""
    import torch

    import bench
    from nvflare_amd import device as device_mod

    monkeypatch.setattr(bench, "PRESETS", dict(bench.PRESETS))
    for name in ("dist_setup", "make_host_helper", "run_client_sharded"):
        monkeypatch.setattr(bench, name, getattr(bench, name))
    for name in ("synchronize", "empty_cache"):
        monkeypatch.setattr(torch.cuda, name, getattr(torch.cuda, name))
    monkeypatch.setattr(device_mod.DeviceContext, "get", device_mod.DeviceContext.__dict__["get"])
    threads = torch.get_num_threads()  # install() runs torch on one thread
    yield
    torch.set_num_threads(threads)


@pytest.mark.timeout(300)
def test_default_run_at_one_gpu(monkeypatch, undo_install):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench = install(0, 1)
    monkeypatch.setattr(bench, "dist_setup", lambda args: (1, 0, 0))
    from nvflare_amd.device import DeviceContext

    ctx = DeviceContext.get(0)
    # room for every preset but config 4's 256-client slab (as one MI355X holds configs 2, 3, 5 but not config 4)
    monkeypatch.setattr(ctx, "total_bytes", bench.HEADROOM + (8 << 20))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main(["--full", "--steps", "2", "--warmup", "1", "--host-resident-params", "10001", "--spot-check", "64",
                    "--cpu-baseline-s", "0.2", "--cpu-sample-params", "4096"])
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    small = small_presets(1)
    assert d["n_gpus"] == 1 and d["spot_check"]["mismatches"] == 0

    def name(e):
        return e.get("baseline_config") or e["config"]["baseline_config"]

    names = [name(e) for e in d["also"]]
    # 2h / 2s / 4x: 2s and 4x skip at one GPU (nothing to split / exchange); every device-resident entry is measured
    measured = [e for e in d["also"] if "roofline" in e]
    assert len(measured) == 3, names
    c2 = next(e for e in measured if e["config"]["clients"] == small[2]["clients"])
    assert c2["config"]["params_total"] == small[2]["params"] and c2["spot_check"]["mismatches"] == 0
    c4 = next(e for e in measured if e["config"]["clients"] == small[4]["clients"])
    from nvflare_amd.sharding import bucket_ranges

    lo, hi = max(bucket_ranges(small[4]["params"], 8), key=lambda b: b[1] - b[0])
    assert "ONE GPU's share of the 8-GPU split" in name(c4)
    assert c4["config"]["share"] == {"of_params_total": small[4]["params"], "gpus": 8, "bucket": [lo, hi]}
    assert c4["config"]["params_total"] == hi - lo and c4["spot_check"]["mismatches"] == 0
    assert c4["value"] == pytest.approx(4.0 * small[4]["clients"] * (hi - lo) / (c4["ms_per_step"] / 1e3) / 2**30,
                                        rel=2e-3, abs=0.006)
    c5 = next(e for e in measured if e["config"]["epilogue"] == "adam")
    assert c5["handout_pull"]["bytes_per_gpu_rank0"] == 4 * small[5]["params"]
    assert not any("skipped" in e and "config 4" in name(e) and "client-sharded" not in name(e) for e in d["also"])
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["n_gpus_in_run"] == 1
    assert set(d["gpu_state"]) == {"before", "main_timed", "after"}


def _plain_line(bench, argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main(argv)
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_plain_run_times_the_steps_and_dumps_its_outputs(monkeypatch, undo_install, tmp_path, oracle):
    """Without --full the run stages, warms up, times --steps steps, writes --dump-outputs and prints the line: no spot
    check, no CPU baseline, no other entries, no GPU state.  The dumped aggregate is the oracle's bit for bit, a second
    run with the same arguments dumps the same bytes, and the fused Adam run dumps the parameter and both moments."""
    import numpy as np

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench = install(0, 1)
    monkeypatch.setattr(bench, "dist_setup", lambda args: (1, 0, 0))
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: pytest.fail("the CPU baseline ran without --full"))
    monkeypatch.setattr(bench, "spot_check", lambda *a, **k: pytest.fail("the spot check ran without --full"))
    monkeypatch.setattr(bench, "handout_pull", lambda *a, **k: pytest.fail("the hand-out pull ran without --full"))
    monkeypatch.setattr(bench, "gpu_monitor", lambda *a, **k: pytest.fail("the GPU monitor started without --full"))
    d = _plain_line(bench, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["metric"] == bench.METRIC
    assert "also" not in d and "spot_check" not in d and d["cpu_baseline"] is None and d["gpu_state"] is None
    small = small_presets(1)[3]
    K, P = small["clients"], small["params"]
    assert d["value"] == pytest.approx(4.0 * K * P / (d["ms_per_step"] / 1e3) / 2**30, rel=2e-3, abs=0.006)
    got = np.load(tmp_path / "a" / "aggregate.npy")
    assert got.dtype == np.float32 and got.shape == (P,)
    cols = np.arange(P, dtype=np.uint64)
    want = oracle.fedavg_c([oracle.synth_values(1000, k, cols) for k in range(K)], oracle.synth_weights(K),
                           oracle.MODE_TORCH)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _plain_line(bench, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "b")])
    assert sorted(os.listdir(tmp_path / "b")) == ["aggregate.npy"]
    assert (tmp_path / "a" / "aggregate.npy").read_bytes() == (tmp_path / "b" / "aggregate.npy").read_bytes()
    _plain_line(bench, ["--config", "5", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "c")])
    assert sorted(os.listdir(tmp_path / "c")) == ["params.npy", "state1.npy", "state2.npy"]
    P5 = small_presets(1)[5]["params"]
    p, m, v = (np.load(tmp_path / "c" / f"{n}.npy") for n in ("params", "state1", "state2"))
    assert p.dtype == m.dtype == v.dtype == np.float32 and p.shape == m.shape == v.shape == (P5,)
    d5 = oracle.fedavg_c([oracle.synth_values(1000, k, np.arange(P5, dtype=np.uint64)) for k in range(64)],
                         oracle.synth_weights(64), oracle.MODE_TORCH)
    p_w = oracle.synth_values(1007, 0, np.arange(P5, dtype=np.uint64))
    m_w, v_w = np.zeros_like(p_w), np.zeros_like(p_w)
    args5 = bench.parse(["--config", "5"])
    for s in (1, 2, 3):  # one warmup step and two timed ones
        oracle.epilogue_apply(d5, oracle.EPI_ADAM, p=p_w, m=m_w, v=v_w, step=float(s),
                              torch_cpu_sqrt=bench.sqrt_mode(args5), **bench.ADAM_HP)
    for got5, want5 in ((p, p_w), (m, m_w), (v, v_w)):
        assert np.array_equal(got5.view(np.uint32), want5.view(np.uint32))


def test_dump_sample_is_fixed_by_the_seed_and_bounded():
    """Arrays beyond DUMP_CHUNKS x DUMP_CHUNK elements are sampled: the same sorted, disjoint, in-range runs for the same
    seed, the first run and the array's tail among them, 16 MiB of float32 per array (three arrays at most: under the
    64 MB a dump may take)."""
    import bench

    limit = bench.DUMP_CHUNK * bench.DUMP_CHUNKS
    assert 3 * 4 * limit <= 64 * 10**6
    for P in (1, 4099, limit):
        assert bench.dump_spans(P, 1000) == [(0, P)]
    for P in (limit + 1, 10**9, 10**9 + 3, 2**31 + 5):
        spans = bench.dump_spans(P, 1000)
        assert spans == bench.dump_spans(P, 1000) and len(spans) == bench.DUMP_CHUNKS
        assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] == P
        assert all(0 < n <= bench.DUMP_CHUNK for _, n in spans)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert sum(n for _, n in spans) <= limit
    assert bench.dump_spans(10**9, 1000) != bench.dump_spans(10**9, 1001)
