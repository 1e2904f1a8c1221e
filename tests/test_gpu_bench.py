"""bench.py end to end on one GPU, in-process on a small mixed-length config: a plain run times the steps and nothing
else, `--dump-outputs` writes the last timed step's outputs (exact against the oracle on the same seeded batch, so two
runs with the same arguments dump the same arrays), and `--full` adds the checks and the other legs."""
import json
import os
import sys

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402

# more frames than bench.DUMP_FRAMES (the dump is a sample), an odd count, lengths that leave a gap to the stride
N, LO, HI, STRIDE, SEED = 300001, 64, 1500, 2048, 0x5EED0B01
W, K = 1, 2


def _bench(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setitem(bench.CONFIGS, "t4", (N, LO, HI, STRIDE, SEED, "t4: test config"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return bench


def _run(bench, monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                                      "--config", "t4", *extra])
    bench.main()
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def expected():
    """The oracle on the W + K batches the run transforms (batch b is global frames b * N ...): the last one's
    outputs, and the counters summed over all of them."""
    totals = dict.fromkeys(("rx_packets", "rx_bytes", "tx_packets", "tx_bytes"), 0)
    for b in range(W + K):
        umem = np.zeros(N * STRIDE, np.uint8)
        descs = oracle.synth_batch(umem, N, 0, STRIDE, SEED, first=b * N, mode=0, len_lo=LO, len_hi=HI)
        verd, recs, st = oracle.echo_batch(umem, descs)
        for k in totals:
            totals[k] += int(st[k])
    return umem, descs, verd, recs, totals


def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(monkeypatch, capsys, tmp_path, expected):
    bench = _bench(monkeypatch)

    def not_in_a_plain_run(*a, **k):
        raise AssertionError("a plain run measures nothing but its steps")

    for leg in ("cpu_baseline", "rx_loop", "host_inclusive", "host_inclusive_multi"):
        monkeypatch.setattr(bench, leg, not_in_a_plain_run)
    monkeypatch.setattr(X, "stream_read_dev", not_in_a_plain_run)
    out = tmp_path / "dump"
    line = _run(bench, monkeypatch, capsys, "--dump-outputs", str(out))

    assert line["metric"] == bench.METRIC and line["unit"] == "Mframes/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == K and line["warmup"] == W
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert line["verified"] is None and line["roofline"]["read_ceiling_gbs"] is None
    assert not {"cpu_baseline", "rx_loop", "host_inclusive", "host_inclusive_multi"} & set(line)

    umem, descs, verd, recs, totals = expected
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {"sample_index", "descs", "verdicts", "records", "frames_index", "frames", "verdict_counts",
                        "record_sums", "stats"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20

    idx = got["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_FRAMES and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < N
    assert (idx == bench.dump_sample(N)).all()
    for j, k in enumerate(X.DESC_DTYPE.names):
        assert (got["descs"][:, j] == descs[k][idx]).all(), k
    assert (got["verdicts"] == verd[idx]).all()
    for j, k in enumerate(X.REC_DTYPE.names):
        assert (got["records"][:, j] == recs[k][idx]).all(), k
        assert got["record_sums"][j] == int(recs[k].astype(np.int64).sum()), k
    assert (got["verdict_counts"] == np.bincount(verd, minlength=256)).all()
    fidx = got["frames_index"].astype(np.int64)
    assert len(fidx) == bench.DUMP_UMEM_FRAMES and np.isin(fidx, idx).all()
    want = umem.reshape(N, STRIDE)[fidx, :bench.DUMP_UMEM_BYTES].copy()
    want[np.arange(bench.DUMP_UMEM_BYTES)[None, :] >= descs["len"][fidx][:, None]] = 0
    assert (got["frames"] == want).all()
    assert got["stats"].tolist() == [totals[k] for k in ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes")]


def test_full_run_checks_every_step_and_adds_the_other_legs(monkeypatch, capsys):
    bench = _bench(monkeypatch)
    monkeypatch.setattr(bench, "cpu_baseline", lambda cfg: {"stub": cfg})
    monkeypatch.setattr(bench, "rx_loop", lambda: {"stub": True})
    line = _run(bench, monkeypatch, capsys, "--full")
    assert line["verified"] is True and line["verification"]["steps_with_outputs_checked"] == W + K
    assert line["roofline"]["read_ceiling_gbs"] > 0 and line["roofline"]["frac_of_read_ceiling"] > 0
    assert line["cpu_baseline"] == {"stub": "t4"} and line["rx_loop"] == {"stub": True}
    assert line["steps"] == K and line["ms_per_step"] > 0

