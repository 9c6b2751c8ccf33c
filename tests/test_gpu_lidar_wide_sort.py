"""kd_lidar_sort_points_wide: the stable point sort by (frame, cell) for BEV grids whose H*W + 1 bins do not fit the LDS
histogram of kd_lidar_sort_points (above 192 x 192 cells).  Checked through the C ABI against numpy's stable argsort and,
where both apply, bit for bit against kd_lidar_sort_points; then through the LiDAR encoder (train and eval take the sorted
"points" form at 200 x 200) and through forward_bf16 at 256 x 256."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu]

RNG = (-50.0, 50.0, -50.0, 50.0)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _inputs(B, N, C, seed, pad=0, dup=0, nan=0, sigma=40.0):           # tests/test_gpu_lidar_segments.py's generator
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, N, 4, generator=g) * torch.tensor([sigma, sigma, 2.0, 1.0])
    if pad:
        pts[:, N - pad:] = 0.0                       # zero padding: all in the cell that holds (0, 0)
    y = torch.randn(B * N, C, generator=g)
    if dup:
        src = torch.randint(0, N - pad - dup, (dup,), generator=g)
        pts[:, N - pad - dup:N - pad] = pts[:, src]  # same cell ...
        yv = y.view(B, N, C)
        yv[:, N - pad - dup:N - pad] = yv[:, src]    # ... and same features: exact ties on every channel
    if nan:
        pts[:, :nan, 0] = float("nan")
        pts[:, nan:2 * nan, 1] = float("inf")
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.2
    mean = torch.randn(C, generator=g) * 0.1
    invstd = torch.rand(C, generator=g) + 0.5
    return [t.cuda().contiguous() for t in (pts.view(B * N, 4), y, sc, sh, mean, invstd)]


def _run(lib, name, pts, B, N, H, W, with_perm=True):
    """One call of a sort entry point on sentinel-filled outputs -> (pts_sorted bits, row_sorted, seg_start, perm) on the host."""
    spts = torch.full((B * N, 4), -5.0, device="cuda")
    srow = torch.full((B * N,), -9, device="cuda", dtype=torch.int32)
    start = torch.full((B * H * W + 1,), -3, device="cuda", dtype=torch.int32)
    perm = torch.full((B * N,), -7, device="cuda", dtype=torch.int32)
    nb = getattr(lib, name + "_ws_bytes")(B, N, H, W)
    ws = torch.full((nb,), 0xA5, device="cuda", dtype=torch.uint8)
    lib.call(name, _P(pts), B, N, H, W, *RNG, _P(spts), _P(srow), _P(start), _P(perm) if with_perm else None, _P(ws), nb, None)
    torch.cuda.synchronize()
    return spts.cpu().numpy().view(np.int32), srow.cpu().numpy(), start.cpu().numpy(), perm.cpu().numpy()


def _check_exact(lib, pts, B, N, H, W):
    spts, srow, start, perm = _run(lib, "kd_lidar_sort_points_wide", pts, B, N, H, W)
    cell = torch.empty(B * N, device="cuda", dtype=torch.int32)
    lib.call("kd_lidar_bev_index", _P(pts), _P(cell), B * N, H, W, *RNG, None)
    torch.cuda.synchronize()
    cell = cell.cpu().numpy().astype(np.int64)
    frame = np.arange(B * N) // N
    key = np.where(cell >= 0, frame * (H * W) + cell, B * H * W + frame)     # out-of-range: after everything, by frame
    want = np.argsort(key, kind="stable")
    assert np.array_equal(perm, want)
    assert np.array_equal(spts, pts.cpu().numpy().view(np.int32)[want])      # bit patterns: NaN coordinates travel unchanged
    assert np.array_equal(srow, np.where(cell >= 0, key, -1)[want])
    counts = np.bincount(key[cell >= 0], minlength=B * H * W)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(counts)]))
    return cell


CASES = [(1, 64, 200, 200, 0, 0, 40.0),            # less than one block
         (1, 1024, 200, 200, 0, 0, 40.0),          # exactly one block
         (1, 1025, 200, 200, 0, 0, 40.0),          # one point into a second block
         (2, 3000, 200, 200, 200, 3, 8.0),         # a padded tail in one cell, NaN and Inf points; many cells hold several points
         (1, 2049, 193, 192, 64, 3, 40.0),         # the first size past the old limit
         (2, 2500, 300, 150, 100, 5, 40.0),        # rectangular
         (2, 2500, 150, 300, 0, 0, 40.0),
         (1, 1500, 10, 4096, 0, 2, 40.0),          # a long axis
         (1, 1500, 4096, 10, 0, 2, 40.0),
         (2, 9000, 256, 256, 0, 13, 8.0),
         (1, 5000, 512, 512, 300, 0, 40.0),
         (3, 3001, 256, 256, 3001, 0, 40.0)]       # every point in one cell


@pytest.mark.parametrize("B,N,H,W,pad,nan,sigma", CASES)
def test_wide_sort_is_the_stable_sort_by_frame_and_cell(B, N, H, W, pad, nan, sigma):
    from kdrt.lib import lib
    pts = _inputs(B, N, 64, 4, pad=pad, nan=nan, sigma=sigma)[0]
    cell = _check_exact(lib, pts, B, N, H, W)
    if sigma == 8.0:
        c0 = cell[:N]                                                        # frame 0
        assert np.bincount(c0[c0 >= 0]).max() >= 3                           # several points per cell: the in-cell order is tested
    if pad == N:
        assert len(np.unique(cell)) == 1 and cell[0] >= 0


def test_wide_sort_with_one_frame_entirely_out_of_range():
    from kdrt.lib import lib
    B, N, H, W = 3, 1500, 200, 200
    pts = _inputs(B, N, 64, 5, pad=100, nan=4)[0]
    pts.view(B, N, 4)[1, :, 0] += 1000.0                                     # frame 1: every x far outside the range
    cell = _check_exact(lib, pts, B, N, H, W)
    assert (cell.reshape(B, N)[1] < 0).all() and (cell.reshape(B, N)[0] >= 0).any() and (cell.reshape(B, N)[2] >= 0).any()


@pytest.mark.parametrize("B,N,H,W,pad,nan", [(3, 5000, 16, 16, 700, 40), (2, 3000, 128, 128, 200, 0), (1, 1500, 192, 192, 0, 2)])
def test_wide_sort_same_bits_as_the_one_level_sort(B, N, H, W, pad, nan):
    from kdrt.lib import lib
    pts = _inputs(B, N, 64, 4, pad=pad, nan=nan)[0]
    a = _run(lib, "kd_lidar_sort_points", pts, B, N, H, W)
    b = _run(lib, "kd_lidar_sort_points_wide", pts, B, N, H, W)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_wide_sort_is_deterministic_and_perm_is_optional():
    from kdrt.lib import lib
    B, N, H, W = 2, 5000, 256, 256
    pts = _inputs(B, N, 64, 6, pad=300, nan=7, sigma=8.0)[0]
    a = _run(lib, "kd_lidar_sort_points_wide", pts, B, N, H, W)
    b = _run(lib, "kd_lidar_sort_points_wide", pts, B, N, H, W)
    c = _run(lib, "kd_lidar_sort_points_wide", pts, B, N, H, W, with_perm=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(a[:3], c[:3]):
        assert np.array_equal(x, y)
    assert (c[3] == -7).all()                                                # perm = NULL: nothing written there


def test_wide_sort_refusals_come_before_any_launch():
    from kdrt.lib import lib
    one = ctypes.c_void_p(16)                        # never dereferenced: every call below is refused before a launch

    def rc(pts=one, spts=one, srow=one, start=one, ws=one, B=1, N=64, H=200, W=200, short=0):
        return lib.kd_lidar_sort_points_wide(pts, B, N, H, W, *RNG, spts, srow, start, None, ws,
                                             lib.kd_lidar_sort_points_wide_ws_bytes(B, N, H, W) - short, None)
    for kw in (dict(H=4097), dict(W=4097), dict(H=4097, W=4097)):
        assert rc(**kw) == -4, kw                                            # KD_ERR_SHAPE
        assert b"4096" in lib.kd_last_error_string()
    assert rc(short=1) == -3                                                 # KD_ERR_WORKSPACE
    for kw in (dict(pts=None), dict(spts=None), dict(srow=None), dict(start=None), dict(ws=None), dict(B=0), dict(N=0), dict(H=0), dict(W=0)):
        assert rc(**kw) == -1, kw                                            # KD_ERR_ARG
    assert lib.kd_lidar_sort_points_wide_ws_bytes(256, 80000, 256, 256) < 1 << 30
    assert lib.kd_lidar_sort_points_wide_ws_bytes(1, 1 << 20, 4096, 4096) < 1 << 30     # no blocks x H*W term


def _record_calls(monkeypatch):
    from kdrt.lib import lib
    calls = []
    real = type(lib).call

    def counting(self, name, *a):
        calls.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(type(lib), "call", counting)
    return calls


def _encoder_run(enc, pts, training):
    enc.zero_grad()
    if not training:
        with torch.no_grad():
            return enc(pts).clone(), []
    y = enc(pts)
    (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
    # (conv biases in front of a BatchNorm have a zero true gradient: rounding noise, not compared)
    return y.detach().clone(), [p.grad.clone() for n, p in enc.named_parameters()
                                if not n.endswith(("point_mlp.0.bias", "point_mlp.3.bias", "point_mlp.6.bias"))]


@pytest.mark.parametrize("training", (False, True))
def test_lidar_encoder_takes_the_sorted_form_on_a_200_x_200_grid(training, monkeypatch):
    """tests/test_gpu_lidar_segments.py's encoder test one size past the one-level sort: eval bit-identical to the atomic
    scatter, train within that test's tolerances and bit-identical from run to run, and the launches are the sorted form's."""
    from kdrt import units
    from src.models.lidar_encoder import LiDAREncoder
    torch.manual_seed(3)
    enc = LiDAREncoder(encoder_type="spatial", grid_size=(200, 200)).cuda().train(training)
    pts = _inputs(2, 6000, 64, 21, pad=500, dup=300, nan=0 if training else 9, sigma=8.0)[0].view(2, 6000, 4)
    calls = _record_calls(monkeypatch)
    res, seen = {}, {}
    for mode in ("atomic", "sorted", "sorted_again", "sorted_narrow"):
        monkeypatch.setattr(units, "_SCATTER_MODE", mode.split("_")[0])
        monkeypatch.setattr(units, "_SORT_WIDE", mode != "sorted_narrow")
        units.clear_step_caches()
        calls.clear()
        res[mode] = _encoder_run(enc, pts, training)
        seen[mode] = list(calls)
    assert "kd_lidar_sort_points_wide" in seen["sorted"] and "kd_lidar_cell_sort" not in seen["sorted"]
    assert "kd_lidar_sort_points" not in seen["sorted"] and "kd_lidar_gather_sorted" not in seen["sorted"]
    if training:
        assert "kd_lidar_seg_hold_fwd" in seen["sorted"] and "kd_lidar_seg_hold_bwd" in seen["sorted"]
    # the switch off: the parent commit's path for such a grid
    assert "kd_lidar_cell_sort" in seen["sorted_narrow"] and "kd_lidar_sort_points_wide" not in seen["sorted_narrow"]
    assert not any(n.startswith("kd_lidar_sort") or n == "kd_lidar_cell_sort" for n in seen["atomic"])
    ya, ys = res["atomic"][0], res["sorted"][0]
    assert (ya > 0).any()
    if training:
        assert torch.allclose(ya, ys, rtol=1e-5, atol=1e-5 * float(ya.abs().max()))
    else:
        assert torch.equal(ya.view(torch.int32), ys.view(torch.int32))
    for mode in ("sorted", "sorted_narrow"):
        for a, b in zip(res["atomic"][1], res[mode][1]):
            assert bool(torch.isfinite(a).all())
            assert torch.allclose(a, b, rtol=2e-5, atol=2e-5 * float(a.abs().max()))
    # a fixed point order: bitwise the same from run to run
    assert torch.equal(ys.view(torch.int32), res["sorted_again"][0].view(torch.int32))
    assert len(res["sorted"][1]) == len(res["sorted_again"][1]) and bool(res["sorted"][1]) == training
    for a, b in zip(res["sorted"][1], res["sorted_again"][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bf16_forward_on_a_256_x_256_grid(monkeypatch):
    """forward_bf16 used to refuse BEV grids above 192 x 192; with the wide sort it runs them, within tests/test_gpu_bf16.py's
    bounds: LOGIT_TOL_REL = 1.5e-2 of the logit range and ARGMAX_MIN = 0.99 against the fp32 HIP forward, 1e-2 of the logit
    range between the one-kernel LiDAR encoder and the layer-by-layer form."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt import KDError, bf16, units
    B, HW, N, G = 2, 128, 5000, 256
    images, pts, _ = O.make_inputs(B, HW, N, G, 5, pad_tail=60)
    images, pts = images.cuda(), pts.cuda()
    model = build_product("concat", G)
    load_random_state(model, "concat", 21)
    model.eval()
    with torch.no_grad():
        z32 = model(images, pts)
    one = bf16.forward_bf16(model, images, pts)
    monkeypatch.setattr(bf16, "_LIDAR_ONE_KERNEL", False)
    two = bf16.forward_bf16(model, images, pts)
    rng = (z32.max() - z32.min()).item()
    assert one.shape == z32.shape and rng > 0
    gap = (one - two).abs().max().item()
    print(f"bf16, 256 x 256 grid: one kernel vs two launches {gap / (two.max() - two.min()).item():.2%} of the logit range")
    assert gap <= 1e-2 * (two.max() - two.min()).item()
    for z16 in (one, two):
        err = (z16 - z32).abs().max().item()
        agree = (z16.argmax(1) == z32.argmax(1)).float().mean().item()
        print(f"bf16 vs fp32 HIP, 256 x 256 grid: max|dlogit| {err / rng:.2%} of range {rng:.2f}, argmax agreement {agree:.4%}")
        assert err <= 1.5e-2 * rng, (err, rng)
        assert agree >= 0.99, agree
    monkeypatch.setattr(units, "_SORT_WIDE", False)
    with pytest.raises(KDError, match="192 x 192"):
        bf16.forward_bf16(model, images, pts)
