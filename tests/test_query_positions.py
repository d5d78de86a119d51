"""Position queries (normals at arbitrary positions, not only at cloud points) without a GPU: the C-ABI declarations, the refusals
that fail before any device call, the argument checks of ``CloudPatches``, the command line's exclusion rule, the data loader's
flag and the ``.qxyz`` reader.  What runs on the device is in tests/test_gpu_query_positions.py."""
import ctypes

import numpy as np
import pytest

import nesti_net_amd  # noqa: F401
from nesti_net_amd import _lib, provider
from nesti_net_amd.config import NestiConfig

NEW_SYMBOLS = ("nesti_patches_query_at", "nesti_estimate_normals_at", "nesti_estimate_normals_multi_at", "nesti_mask_empty_queries")
FAKE = ctypes.c_void_p(4096)      # a non-NULL pointer for arguments a refusal must never dereference
BIG = 1 << 40                     # "large enough" workspace size for the size checks that come before the refusal under test


def _last_error(lib):
    return lib.nesti_last_error().decode()


def test_ctypes_declarations_exist_and_mirror_the_index_forms():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    S = _lib.SIGNATURES
    assert S["nesti_patches_query_at"] == S["nesti_patches_query"]                      # a float* where the int32* was
    assert len(S["nesti_estimate_normals_at"][1]) == len(S["nesti_estimate_normals"][1]) + 1   # + n_ball_out_dev
    assert len(S["nesti_estimate_normals_multi_at"][1]) == len(S["nesti_estimate_normals_multi"][1])
    assert len(S["nesti_mask_empty_queries"][1]) == 8
    # the item struct: the same layout with the positions where the indices were
    assert [f[0] for f in _lib.CShapePositions._fields_] == \
        [f[0].replace("query_idx_dev", "query_xyz_dev") for f in _lib.CShapeQueries._fields_]
    assert ctypes.sizeof(_lib.CShapePositions) == ctypes.sizeof(_lib.CShapeQueries)


def _query_at(lib, cfg, xyz, M, row0=0, r=(0.1, 0.2, 0.3), N=100, ws_bytes=BIG):
    rr = (ctypes.c_double * len(r))(*r)
    c = cfg.to_c()
    return lib.nesti_patches_query_at(ctypes.byref(c), FAKE, N, xyz, M, rr, ctypes.c_uint64(1), row0, None, None, None, None, FAKE,
                                      ws_bytes, None)


def test_patches_query_at_refusals_before_any_device_call():
    lib, cfg = _lib.load(), NestiConfig()
    assert _query_at(lib, cfg, None, 5) != 0
    assert _last_error(lib) == "nesti_patches_query_at: null query_xyz_dev"
    assert _query_at(lib, cfg, FAKE, 5, row0=-1) != 0
    assert _last_error(lib) == "nesti_patches_query_at: query_row0 must be >= 0"
    # everything the index form refuses, in its style
    assert _query_at(lib, cfg, FAKE, 5, N=0) != 0 and _last_error(lib) == "nesti_patches_query_at: empty cloud"
    assert _query_at(lib, cfg, FAKE, 5, ws_bytes=16) != 0 and _last_error(lib) == "nesti_patches_query_at: grid workspace too small"
    assert _query_at(lib, cfg, FAKE, 5, r=(0.1, 0.0, 0.3)) != 0 and _last_error(lib) == "nesti_patches_query_at: radii must be positive and finite"
    assert _query_at(lib, NestiConfig(num_point=1024), FAKE, 5) != 0
    assert _last_error(lib) == "nesti_patches_query_at: points_per_scale must be in [1, 512]"
    c = cfg.to_c()
    assert lib.nesti_patches_query_at(ctypes.byref(c), None, 100, FAKE, 5, None, 0, 0, None, None, None, None, None, 0, None) != 0
    assert _last_error(lib) == "nesti_patches_query_at: null argument"
    # no queries: nothing to do, whatever the pointer; and a position query has no row range to exceed
    assert _query_at(lib, cfg, None, 0) == 0


def test_the_index_form_keeps_its_refusals():
    lib, cfg = _lib.load(), NestiConfig()
    c, rr = cfg.to_c(), (ctypes.c_double * 3)(0.1, 0.2, 0.3)
    assert lib.nesti_patches_query(ctypes.byref(c), FAKE, 100, None, 5, rr, 1, 96, None, None, None, None, FAKE, BIG, None) != 0
    assert _last_error(lib) == "nesti_patches_query: query rows [query_row0, query_row0 + M) exceed the cloud (N points)"
    assert lib.nesti_patches_query(ctypes.byref(c), FAKE, 100, None, 5, rr, 1, -1, None, None, None, None, FAKE, BIG, None) != 0
    assert _last_error(lib) == "nesti_patches_query: query_row0 must be >= 0"


def test_estimate_at_and_mask_refusals_before_any_device_call():
    lib = _lib.load()
    rr = (ctypes.c_double * 3)(0.1, 0.2, 0.3)

    def est(m, xyz, M=5, row0=0):
        return lib.nesti_estimate_normals_at(m, FAKE, 100, xyz, M, rr, ctypes.c_uint64(1), row0, 16, 0, FAKE, BIG, FAKE, BIG, FAKE,
                                             None, None, None, None)
    assert est(None, FAKE) != 0 and _last_error(lib) == "nesti_estimate_normals_at: null argument"
    assert est(FAKE, None) != 0 and _last_error(lib) == "nesti_estimate_normals_at: null query_xyz_dev"
    assert est(FAKE, FAKE, row0=-3) != 0 and _last_error(lib) == "nesti_estimate_normals_at: query_row0 must be >= 0"
    assert est(None, None, M=0) == 0
    items = (_lib.CShapePositions * 1)()
    items[0].n_queries = 4
    assert lib.nesti_estimate_normals_multi_at(None, items, 1, 16, FAKE, BIG, FAKE, None, None, None) != 0
    assert _last_error(lib) == "nesti_estimate_normals_multi_at: null argument"
    items[0].n_queries = 0
    assert lib.nesti_estimate_normals_multi_at(None, items, 1, 16, None, 0, None, None, None, None) == 0
    assert lib.nesti_mask_empty_queries(None, 4, 3, FAKE, None, None, 7, None) != 0
    assert _last_error(lib) == "nesti_mask_empty_queries: null argument"
    assert lib.nesti_mask_empty_queries(FAKE, 4, 0, FAKE, None, None, 7, None) != 0
    assert _last_error(lib) == "nesti_mask_empty_queries: bad n_scales"
    assert lib.nesti_mask_empty_queries(FAKE, 4, 3, FAKE, None, FAKE, 0, None) != 0
    assert _last_error(lib) == "nesti_mask_empty_queries: probs_dev needs E >= 1 columns"
    assert lib.nesti_mask_empty_queries(None, 0, 3, None, None, None, 7, None) == 0


def test_cloud_patches_argument_checks():
    """All of them are raised before the library or the device is touched."""
    cfg = NestiConfig()
    pts = np.random.RandomState(0).rand(50, 3).astype(np.float32)
    q = pts[:4] + 0.01
    with pytest.raises(ValueError, match="mutually exclusive"):
        provider.CloudPatches(pts, cfg, pidx=[0, 1], queries=q)
    for bad in (np.zeros(3, np.float32), np.zeros((4, 2), np.float32), np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"queries must be \[M,3\]"):
            provider.CloudPatches(pts, cfg, queries=bad)
    for v in (np.nan, np.inf, -np.inf):
        b = q.astype(np.float64)
        b[2, 1] = v
        b[3, 0] = v
        with pytest.raises(ValueError, match="queries row 2 is not finite"):
            provider.CloudPatches(pts, cfg, queries=b)
    ok = provider.check_queries([[0, 1, 2], [3, 4, 5]])
    assert ok.dtype == np.float32 and ok.shape == (2, 3) and ok.flags["C_CONTIGUOUS"]
    assert provider.check_queries(np.zeros((0, 3))).shape == (0, 3)


def test_command_line_refuses_positions_with_sparse_patches(tmp_path, capsys):
    from nesti_net_amd.cli import build_parser, main
    assert build_parser().parse_args([]).query_positions == 0
    with pytest.raises(SystemExit) as e:
        main(["--results_path", str(tmp_path / "log"), "--query_positions", "1", "--sparse_patches", "1"])
    assert e.value.code == 2 and "mutually exclusive" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(["--results_path", str(tmp_path / "log"), "--query_positions", "1", "--subsample", "reference"])
    assert e.value.code == 2 and "--subsample hash" in capsys.readouterr().err
    assert not (tmp_path / "log").exists()      # refused before anything is created


def test_get_data_loader_passes_the_flag_through(monkeypatch):
    seen = []

    class FakeDataset:
        def __init__(self, root, listfile, cfg, **kw):
            seen.append(kw)
            self.shape_names, self.shape_patch_count = [], []

        def __len__(self):
            return 0

    monkeypatch.setattr(provider, "PointcloudPatchDataset", FakeDataset)
    for flag in (False, True):
        provider.get_data_loader("list.txt", 8, "/nowhere", [0.01, 0.03, 0.05], 512, query_positions=flag)
        assert seen[-1]["query_positions"] is flag and seen[-1]["sparse_patches"] is False
    provider.get_data_loader("list.txt", 8, "/nowhere", [0.01, 0.03, 0.05], 512)
    assert seen[-1]["query_positions"] is False


def test_dataset_refuses_both_query_kinds(tmp_path):
    (tmp_path / "list.txt").write_text("")
    with pytest.raises(ValueError, match="mutually exclusive"):
        provider.PointcloudPatchDataset(str(tmp_path), "list.txt", NestiConfig(), sparse_patches=True, query_positions=True)


def test_qxyz_reader(tmp_path):
    one = tmp_path / "one.qxyz"
    one.write_text("0.5 -1.25 3e-2\n")
    q = provider.load_qxyz(str(one))
    assert q.dtype == np.float32 and q.shape == (1, 3) and q.tolist() == [[0.5, -1.25, np.float32(3e-2)]]
    many = tmp_path / "many.qxyz"
    ref = np.random.RandomState(1).randn(7, 3).astype(np.float32)
    np.savetxt(str(many), np.concatenate([ref, np.ones((7, 3), np.float32)], axis=1), fmt="%.9g")     # extra columns are ignored, like .xyz
    q = provider.load_qxyz(str(many))
    assert q.shape == (7, 3) and np.array_equal(q, ref) and q.flags["C_CONTIGUOUS"]
    assert not (tmp_path / "many.qxyz.npy").exists()
