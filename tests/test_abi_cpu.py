"""CPU-side checks of the boundary: the C-ABI library loads, exports every symbol that
include/slam_hip.h declares, and refuses to run without a GPU (no CPU fallback); plus the
host logic that needs no device (parameters, synthetic streams, index-rule helpers)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, pkg


def test_library_exports_every_declared_symbol():
    abi = pkg("_abi")
    L = abi.lib()
    names = abi.header_symbols()
    assert len(names) >= 30 and "slam_replay_dev" in names and "slam_icp_batch" in names
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert set(abi._SIGS) == set(names)          # the ctypes binding covers the whole header
    assert L.slam_abi_version() == 1


SYNTHETIC_HEADER = """
/* int commented_out(int a); */
// double also_commented_out(void);
#ifdef __cplusplus
extern "C" {
#endif
#define NOT_A_CALL(x) (x)
typedef struct thing thing;
enum { A = 0, B = 4 };
int by_value(int a, double b, float c, int64_t d);
int pointers(const double *in, thing **out, int32_t x[4], const int32_t y[2][2], void *raw);
int no_arguments(void);
const char *text(void);
int takes_text(thing *t, const char *name, char **names);
double wrapped(thing *t,   /* a comment inside the list */
               const float *ranges, int n,
               int64_t
                   count);
int unnamed(int, const float *, double);
#ifdef __cplusplus
}
#endif
"""


def test_signatures_are_parsed_from_the_header_by_the_type_rule():
    abi = pkg("_abi")
    vp, i, d, f, i64, s = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_int64, C.c_char_p
    assert abi.header_signatures(text=SYNTHETIC_HEADER) == {
        "by_value": ([i, d, f, i64], i),
        "pointers": ([vp, vp, vp, vp, vp], i),
        "no_arguments": ([], i),
        "text": ([], s),
        "takes_text": ([vp, s, vp], i),
        "wrapped": ([vp, vp, i, i64], d),
        "unnamed": ([i, vp, d], i),
    }
    for bad in ("int f(long n);", "int f(unsigned int n);", "int f(size_t n);", "long f(int n);", "void f(int n);", "int f(int32_t n);",
                "int f(int (*callback)(int));"):
        with pytest.raises(abi.SlamError, match=r"\bf\b"):
            abi.header_signatures(text="int good(int a);\n" + bad)


def test_real_header_widths_where_a_slip_would_corrupt_arguments():
    """Positions counted in include/slam_hip.h itself: a float bound as a double, or an int64_t bound as an int, shifts or
    truncates every argument after it without any error."""
    abi = pkg("_abi")
    sig = abi.header_signatures()
    assert sig == abi._SIGS and len(sig) == 95
    vp, i, d, f, i64 = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_int64
    for name in ("slam_grid_match", "slam_grid_match_dev"):
        args = sig[name][0]
        assert args[11:17] == [i, i, i, d, f, i], name              # K, nx, ny, double step, float max_range, cap
    for name in ("slam_grid_raycast", "slam_grid_raycast_dev"):
        assert sig[name][0][7:10] == [i, f, i], name                # n, float max_range, skip
    assert sig["slam_bresenham_batch"][0] == [vp, vp, vp, i, vp, vp, vp, i64]                      # int64_t total_cells, last
    for name in ("slam_ekf_lm", "slam_ekf_lm_dev"):
        assert sig[name][0][5:8] == [vp, i64, i], name              # z, int64_t nz, B
    assert sig["slam_loc_replay_dev"][0][9:12] == [i, i64, vp]      # M, int64_t K, map_of_traj
    assert i64 not in sig["slam_loc_replay"][0]                     # (the host form reads K from obs_off[M])
    assert sig["slam_last_error"] == ([], C.c_char_p) and sig["slam_set_option"][0] == [vp, C.c_char_p, d]
    assert all(res is i for name, (_a, res) in sig.items() if name != "slam_last_error")


def test_header_cites_reference_for_every_operator():
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    for ref in ("icp.py:38-88", "icp.py:90-114", "icp.py:149-179", "mapping.py:22-51", "mapping.py:8-20",
                "bresenham.py:2-58", "slam_ekf.py:63-95", "slam_ekf.py:270-271", "icp.py:153-158"):
        assert ref in text, ref
    assert not re.search(r"\btorch\b|at::Tensor", text.split("Conventions")[1].split("#ifndef")[0].replace("torch.Tensor.data_ptr()", ""))


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    slam = pkg()
    with pytest.raises(slam.SlamError, match="no HIP device|no CPU path"):
        slam.ICP()
    with pytest.raises(slam.SlamError):
        slam.Mapping(200, 200, 0.1)
    with pytest.raises(slam.SlamError):
        slam.bresenham([0, 0], [3, 1])
    with pytest.raises(slam.SlamError):
        slam.DeviceReplay(np.zeros((3, 8), dtype=np.float32), -3.0, 3.0)
    # identical endpoints never reach the device (bresenham.py:10-11)
    assert slam.bresenham([2, 2], [2, 2]).path == []


def test_product_never_uses_the_oracle():
    """Nothing under the package imports, loads or links anything from oracle/."""
    pkg_dir = os.path.join(ROOT, PKG)
    pat = re.compile(r"import\s+oracle|from\s+oracle|liboracle|oracle[/\\]|c_oracle|oracle_np|slam_oracle")
    for dp, _dn, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                txt = open(os.path.join(dp, f)).read()
                assert not pat.search(txt), f


def test_null_and_bad_arguments_are_rejected_before_any_device_work():
    abi = pkg("_abi")
    L = abi.lib()
    assert L.slam_create(0, None, None) == abi.ERR_INVALID
    assert b"out is null" in L.slam_last_error()
    assert L.slam_synchronize(None) == abi.ERR_INVALID
    assert L.slam_destroy(None) == abi.SLAM_OK
    h = C.c_void_p()
    assert L.slam_grid_create(None, 1, 10, 10, 10.0, 10.0, 10.0, 0.01, 20.0, 10.0, C.byref(h)) == abi.ERR_INVALID


def test_params_table():
    p = pkg("param")
    p.clear_params()
    assert p.get_param('/icp/max_iter', 30) == 30
    p.set_param('/icp/max_iter', 10)
    assert p.get_param('/icp/max_iter', 30) == 10
    p.clear_params()
    with pytest.raises(KeyError):
        p.get_param('/slam/map_width')


def test_synthetic_streams_are_deterministic_and_in_spec(syn):
    a, b = syn.make_replay(12, 120, seed=5, stride=5), syn.make_replay(12, 120, seed=5, stride=5)
    assert np.array_equal(a.ranges, b.ranges) and a.ranges.dtype == np.float32 and a.ranges.shape == (12, 120)
    assert a.ranges.min() >= 0.1 and a.ranges.max() <= 30.0
    assert not np.array_equal(a.ranges, syn.make_replay(12, 120, seed=6, stride=5).ranges)
    step = np.hypot(*np.diff(a.poses_true[:, :2], axis=0).T)
    assert np.allclose(step, 0.15, atol=2e-3)            # 0.3 m/s, every 5th message of 10 Hz
    m = a.message(3)
    assert isinstance(m.ranges, tuple) and m.angle_min == -3.14159 and len(m.ranges) == 120
    pri = syn.particle_priors(1000, seed=2)
    assert abs(pri[:, 0].std() - 0.05) < 0.005 and abs(pri[:, 2].std() - np.deg2rad(2)) < 0.004


def test_trig_tables_match_reference_formula():
    abi = pkg("_abi")
    ct, st = abi.trig_tables(-3.14159, 3.14159, 360)
    ang = np.linspace(-3.14159, 3.14159, 360)
    assert np.array_equal(ct, np.cos(ang)) and np.array_equal(st, np.sin(ang))
