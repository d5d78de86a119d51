"""Reproducible mode, the parts that need no GPU: the deterministic gate margin (calibrate.reproducible_gate_margin), the
null-handle behaviour of the two new entry points, and the multi-rank verified loop (dist.estimate_sharded over
pipeline.verified_passes) on a world-2 gloo group with a stand-in estimator whose ranks measure different things."""
import ctypes
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO


def test_margin_is_the_widening_factor_when_the_shape_is_the_sample():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.calibrate import reproducible_gate_margin
    # n_t = max(n_s, (E - 1) x shape_queries) = n_s: growth 1, tau = NESTI_GATE_WIDEN x max_err
    assert reproducible_gate_margin(0.1, 6144, 1024, 7) == pytest.approx(0.15, rel=1e-12)
    assert reproducible_gate_margin(0.1, 6144, 10, 7) == pytest.approx(0.15, rel=1e-12)      # a shape smaller than the sample


def test_margin_grows_like_a_gaussian_maximum():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.calibrate import reproducible_gate_margin
    growth = math.sqrt(math.log(600000) / math.log(6144))
    assert reproducible_gate_margin(0.08, 6144, 100000, 7) == pytest.approx(1.5 * growth * 0.08, rel=1e-12)
    taus = [reproducible_gate_margin(0.08, 6144, n, 7) for n in (100, 1024, 1025, 5000, 100000, 10 ** 7)]
    assert all(a <= b for a, b in zip(taus, taus[1:])) and taus[1] < taus[2] < taus[-1]      # monotone in shape_queries


def test_margin_floor_and_purity():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd.calibrate import reproducible_gate_margin
    assert reproducible_gate_margin(0.0, 6144, 100000, 7) == 1e-3
    assert reproducible_gate_margin(1e-5, 6144, 100000, 7, floor=0.05) == 0.05
    assert reproducible_gate_margin(0.3, 6144, 100000, 7, floor=0.05) > 0.45
    a = [reproducible_gate_margin(0.0731, 6144, 99991, 7) for _ in range(3)]
    assert a[0] == a[1] == a[2]                                                              # identical inputs, identical bits


def test_null_handle_is_refused_with_a_message():
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import _lib
    lib = _lib.load()
    assert lib.nesti_model_set_reproducible(None, 1) != 0
    assert b"nesti_model_set_reproducible" in lib.nesti_last_error()
    st = _lib.CReproducibleStats()
    assert lib.nesti_model_reproducible_stats(None, ctypes.byref(st), 0, None) != 0
    assert b"nesti_model_reproducible_stats" in lib.nesti_last_error()
    with pytest.raises(_lib.NestiError, match="nesti_model_set_reproducible"):
        _lib.check(lib.nesti_model_set_reproducible(None, 0), "nesti_model_set_reproducible")
    # the guard twins of the gate error pair refuse a null handle too
    assert lib.nesti_model_guard_error_export(None, None, None) != 0 and lib.nesti_model_guard_error_import(None, None, 0, None) != 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _FakeCloud:
    def __init__(self, n):
        self.patch_count = n


class _FakeReproducibleEstimator:
    """Stands in for NormalEstimator(..., reproducible=True): its rows are a function of (row, tau, thr), and what it "measures"
    depends on the RANK -- ``err`` / ``dn`` per rank, a violation whenever 1.5 x the rank's value exceeds the threshold."""
    reproducible = True
    subsample = "hash"

    def __init__(self, err, dn, tau=0.1, thr=0.05, scale=100.0):
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # noqa: E731 -- measured values are float32 on the device
        self.err, self.dn, self.tau, self.thr, self.scale = f32(err), f32(dn), tau, thr, scale
        self.runs, self.last_verified = 0, None

    def run(self, cloud, first, count):
        self.runs += 1
        rows = torch.arange(first, first + count, dtype=torch.float32)
        return (torch.stack([rows, rows + self.tau, rows + self.thr], 1), (torch.arange(first, first + count) % 7).to(torch.int32),
                torch.stack([rows + e for e in range(7)], 1))

    def run_many(self, items):
        self.runs -= len(items) - 1                      # one pass, however many shapes
        return [self.run(c, f, n) for c, f, n in items]

    def verify_begin(self):
        return (self.tau, self.thr)

    def verify_flags(self):
        violated = 1.5 * self.err > self.tau or self.scale * self.dn > self.thr
        return torch.tensor([self.err, self.dn, float(violated), 0.0], dtype=torch.float32)

    def verify_raise(self, err, dn):
        self.tau, self.thr = max(self.tau, 1.5 * err), max(self.thr, self.scale * dn)

    def verify_record(self, passes, err, dn):
        self.last_verified = {"passes": passes, "tau": self.tau, "thr": self.thr, "max_margin_err": err, "max_dn": dn}

    def verify_end(self, saved):
        self.tau, self.thr = saved


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, REPO)
    import nesti_net_amd  # noqa: F401
    from nesti_net_amd import dist as nd
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # rank 0 stays inside its margin (1.5 x 0.05 < 0.1) but shows the larger |dn|; rank 1 violates the margin only
    est = _FakeReproducibleEstimator(err=(0.05, 0.08)[rank], dn=(6e-4, 1e-4)[rank])
    n, e, p = nd.estimate_sharded(est, _FakeCloud(1001))
    one = dict(est.last_verified, runs=est.runs, restored=(est.tau, est.thr), col1=float(n[1000, 1] - n[1000, 0]),
               col2=float(n[0, 2] - n[0, 0]), rows=len(n))
    # nobody violates: one pass, and no thresholds move
    quiet = _FakeReproducibleEstimator(err=0.01, dn=1e-5)
    nd.estimate_sharded_many(quiet, [_FakeCloud(64), _FakeCloud(5)])
    # a rank that keeps violating: every rank gives up after the same number of passes, thresholds restored
    class _Never(_FakeReproducibleEstimator):
        def verify_flags(self):
            return torch.tensor([self.err, self.dn, float(rank == 1), 0.0], dtype=torch.float32)
    never = _Never(err=0.5, dn=0.0)
    try:
        nd.estimate_sharded(never, _FakeCloud(10))
        gave_up = None
    except Exception as ex:      # noqa: BLE001 -- reported to the parent
        gave_up = type(ex).__name__
    q.put((rank, one, dict(quiet.last_verified, runs=quiet.runs), gave_up, never.runs, (never.tau, never.thr)))
    dist.barrier()
    dist.destroy_process_group()


def test_both_ranks_take_the_same_passes_and_thresholds_world_2():
    from nesti_net_amd import _lib
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # noqa: E731 -- the maxima travel as float32
    for rank, one, quiet, gave_up, never_runs, never_thr in res:
        # pass 1: rank 1 violates the margin, rank 0 the guard; both re-run with the GLOBAL maxima of both quantities
        assert one["passes"] == 2 and one["runs"] == 2, (rank, one)
        assert one["tau"] == pytest.approx(1.5 * f32(0.08), rel=1e-12) and one["thr"] == pytest.approx(100.0 * f32(6e-4), rel=1e-12)
        assert one["max_margin_err"] == f32(0.08) and one["max_dn"] == f32(6e-4)
        assert one["restored"] == (0.1, 0.05) and one["rows"] == 1001
        # the gathered rows of BOTH shards were computed with the raised thresholds
        assert one["col1"] == pytest.approx(one["tau"], abs=1e-3) and one["col2"] == pytest.approx(one["thr"], abs=1e-6)
        assert quiet["passes"] == 1 and quiet["runs"] == 1 and quiet["tau"] == 0.1
        assert gave_up == "NestiError" and never_runs == 1 + _lib.GATE_WIDEN_PASSES and never_thr == (0.1, 0.05)
    assert res[0][1] == res[1][1]
