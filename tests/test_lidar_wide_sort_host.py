"""CPU tests of the host side of the wide LiDAR point sort (kd_lidar_sort_points_wide, for BEV grids above 192 x 192 cells): the
C ABI of the two entry points (declared in include/kd_hip.h, exported by the built library), the refusals that return before
any launch, the workspace bound, and the KD_LIDAR_WIDE_SORT switch of kdrt.units."""
import ctypes
import os
import re
import subprocess
import sys

RNG = (-50.0, 50.0, -50.0, 50.0)


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_lidar_sort_points_wide", "kd_lidar_sort_points_wide_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    # the same argument list as the one-level sort
    assert protos["kd_lidar_sort_points_wide"] == protos["kd_lidar_sort_points"]
    assert protos["kd_lidar_sort_points_wide_ws_bytes"] == protos["kd_lidar_sort_points_ws_bytes"]


def test_workspace_query_and_argument_errors():
    from kdrt.lib import lib
    ws_bytes = lib.kd_lidar_sort_points_wide_ws_bytes
    assert ws_bytes(256, 80000, 256, 256) < 1 << 30
    # no term proportional to blocks x H*W: the one-level sort's table alone would be 5.3 GB here
    assert lib.kd_lidar_sort_points_ws_bytes(256, 80000, 256, 256) > 5 << 30
    # 4 ints per point, (W + H + 1) per block and per frame, one per frame, one per 2048 cells (+ 1)
    B, N, H, W = 3, 2500, 300, 150
    assert ws_bytes(B, N, H, W) == 4 * (4 * B * N + B * 3 * (W + H + 1) + B * (W + H + 1) + B + (B * H * W + 1 + 2047) // 2048)
    one = ctypes.c_void_p(16)                        # never dereferenced: every call below is refused before a launch

    def rc(pts=one, spts=one, srow=one, start=one, ws=one, B=1, N=64, H=200, W=200, short=0):
        return lib.kd_lidar_sort_points_wide(pts, B, N, H, W, *RNG, spts, srow, start, None, ws, ws_bytes(B, N, H, W) - short, None)
    for kw in (dict(pts=None), dict(spts=None), dict(srow=None), dict(start=None), dict(ws=None), dict(B=0), dict(N=0), dict(H=0), dict(W=0)):
        assert rc(**kw) == -1, kw                                            # KD_ERR_ARG
        assert b"kd_lidar_sort_points_wide" in lib.kd_last_error_string()
    for kw in (dict(H=4097), dict(W=4097)):
        assert rc(**kw) == -4, kw                                            # KD_ERR_SHAPE, naming the limit
        assert b"4096" in lib.kd_last_error_string()
    assert rc(B=1 << 15, N=1 << 16) == -4                                    # 2^31 points
    assert rc(B=1 << 8, H=4096, W=4096) == -4                                # 2^31 cells
    assert rc(short=1) == -3                                                 # KD_ERR_WORKSPACE


def test_switch_is_read_from_the_environment_once():
    from kdrt import units
    assert units._SORT_WIDE is (os.environ.get("KD_LIDAR_WIDE_SORT", "1") != "0")
    assert units.sorted_mode_available(192, 192)
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(units.__file__)))
    code = ("from kdrt import units; "
            "print(units._SORT_WIDE, units.sorted_mode_available(192, 192), units.sorted_mode_available(193, 192), "
            "units.sorted_mode_available(4096, 4096), units.sorted_mode_available(10, 4097))")
    flags = ["-s"] if sys.flags.no_user_site else []
    env = dict(os.environ, KD_LIDAR_WIDE_SORT="0")
    env["PYTHONPATH"] = os.pathsep.join([pkg] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "False True False False False", r.stdout
    if units._SORT_WIDE:                             # the default: on, up to 4096 cells per side
        assert units.sorted_mode_available(193, 192) and units.sorted_mode_available(4096, 4096)
        assert not units.sorted_mode_available(10, 4097)
