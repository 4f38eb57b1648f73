"""Steps 2b, 4s and 7 of the Poisson reconstruction (include/vslam_abi.h; csrc/poisson_screen.hip and the variants in
csrc/cloud_poisson.hip) against numpy fp64: the density, the screened system's true residual restated from the returned
fields, and the trimmed mesh as the surviving part of the untrimmed one."""
import numpy as np
import pytest

import vslam_abi
from test_gpu_poisson import KINDS, at, closed, ref_grid, ref_iso_value, ref_solve, ref_trilinear, shell, slab

pytestmark = pytest.mark.gpu

TOL = 1e-10
_runs = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def splat(q, w, R):
    W = np.zeros((R, R, R))
    np.add.at(W, (q[..., 2], q[..., 1], q[..., 0]), w)
    return W


@pytest.mark.parametrize("R", [16, 21, 65])
def test_density(vsctx, R):
    p, N = slab(R)[:2]
    W = splat(*ref_trilinear(p, *ref_grid(p, R), R), R)
    runs = [vsctx.cloud_poisson(p, N, fields=True, density=True, resolution=R, max_iter=1)["density"] for _ in range(2)]
    err = np.abs(runs[0] - W).max() / W.max()
    print("R", R, "density error / max W", err)
    assert err <= 1e-12
    assert np.array_equal(bits(runs[0]), bits(runs[1]))


def screened(vsctx, R, solver):
    if (R, solver) not in _runs:
        p, N = slab(R)[:2]
        _runs[R, solver] = [vsctx.cloud_poisson(p, N, fields=True, resolution=R, solver=solver, tol=TOL, point_weight=pw)
                            for pw in (6.0, 6.0, 0.0)]
    return _runs[R, solver]


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("R", [16, 17, 21, 33])  # 17, 21, 33: the sine transform's ragged tiles
def test_screened(vsctx, R, solver):
    p = slab(R)[0]
    out, again, plain = screened(vsctx, R, solver)
    o, h = ref_grid(p, R)
    q, w = ref_trilinear(p, o, h, R)
    rhs, chi, info = out["rhs"], out["chi"], out["info"]
    chi0, cond = ref_solve(rhs, h)
    tau = ref_iso_value(chi0, p, o, h)
    cells = len(np.unique((q[:, 0, 2] * R + q[:, 0, 1]) * R + q[:, 0, 0]))
    lam = 6.0 / (h * h * (len(p) / cells))
    x = np.pad(chi, 1)
    c = slice(1, -1)
    Ax = (6 * chi - (x[c, c, :-2] + x[c, c, 2:] + x[c, :-2, c] + x[c, 2:, c] + x[:-2, c, c] + x[2:, c, c])) / (h * h)
    Bx = (w * at(chi, q)).sum(1)
    b = -rhs + lam * tau * splat(q, w, R)
    res = np.linalg.norm(Ax + lam * splat(q, w * Bx[:, None], R) - b) / np.linalg.norm(b)
    print("R", R, "solver", solver, "iterations", info[0], "true residual", res, "reported", info[1], "cond", cond)
    assert res <= 2 * TOL
    assert info[3] == 1 and info[0] > 0 and info[1] <= TOL
    assert abs(info[2] - ref_iso_value(chi, p, o, h)) <= 1e-12 * np.abs(chi).max()  # a mean of values of chi
    other = screened(vsctx, R, 1 - solver)[0]["chi"]
    assert np.linalg.norm(chi - other) <= 2 * cond * TOL * np.linalg.norm(chi)
    assert again["info"][0] == info[0] and np.array_equal(bits(again["chi"]), bits(chi))
    off = np.abs((w * at(plain["chi"], q)).sum(1) - plain["info"][2]).mean()
    print("mean |B chi - iso|: screened", np.abs(Bx - info[2]).mean(), "plain", off)
    assert np.abs(Bx - info[2]).mean() < off


@pytest.mark.parametrize("pw", [0.0, 6.0])
def test_trim(vsctx, pw):
    p, No = shell()[0], shell()[3]
    keep = p[:, 2] < np.sort(p[:, 2])[-(len(p) // 6)]  # without the top sixth: an open surface
    p, No, R = p[keep], No[keep], 32
    call = lambda **kw: vsctx.cloud_poisson(p, No, fields=True, density=True, resolution=R, solver=1, tol=TOL,  # noqa: E731
                                            point_weight=pw, **kw)
    full = call()
    chi, iso, W = full["chi"], full["info"][2], full["density"]
    below = chi < iso
    keys = []
    for kind, (dx, dy, dz) in enumerate(KINDS):
        k, j, i = np.nonzero(below[:R - dz, :R - dy, :R - dx] != below[dz:, dy:, dx:])
        keys.append(7 * ((k * R + j) * R + i) + kind)
    keys = np.sort(np.concatenate(keys))
    a = np.stack([keys // 7 % R, keys // 7 // R % R, keys // 7 // (R * R)], 1)
    b = a + np.array(KINDS)[keys % 7]
    t = (iso - at(chi, a)) / (at(chi, b) - at(chi, a))
    rho = at(W, a) + t * (at(W, b) - at(W, a))
    assert full["counts"][0] == len(rho) and np.abs(full["vert_density"] - rho).max() <= 1e-12 * W.max()
    srt = np.sort(rho)
    trim = (srt[len(rho) // 2 - 1] + srt[len(rho) // 2]) / 2  # the median, between two neighbours
    assert np.abs(rho - trim).min() >= 1e-9 * W.max(), "a vertex lies on the threshold: pick another seed"
    alive = rho >= trim
    tkeep = alive[full["tri"]].all(1)
    cut = call(trim=trim)
    print("point_weight", pw, "trim", trim, "counts", full["counts"].tolist(), "->", cut["counts"].tolist())
    assert cut["counts"].tolist() == [alive.sum(), tkeep.sum()]
    assert np.array_equal(bits(cut["verts"]), bits(full["verts"][alive]))
    assert np.array_equal(bits(cut["vert_density"]), bits(full["vert_density"][alive]))
    assert np.array_equal(cut["tri"], (np.cumsum(alive) - 1)[full["tri"][tkeep]])
    assert closed(full["tri"]) and not closed(cut["tri"])


def test_arguments(vsctx):
    p, N = slab(16)[:2]
    for field in ("point_weight", "trim"):
        for bad in (-1.0, float("nan")):
            with pytest.raises(vslam_abi.VSError, match="VS_ERR_ARG"):
                vsctx.cloud_poisson(p, N, resolution=16, **{field: bad})
    for solver in (0, 1):
        out = vsctx.cloud_poisson(p, np.zeros_like(N), fields=True, resolution=16, solver=solver, point_weight=6.0)
        assert out["counts"].tolist() == [0, 0] and out["info"][0] == 0 and not out["chi"].any()
        assert np.all(np.isfinite(out["info"]))
    big = vsctx.cloud_poisson(p, N, fields=True, density=True, resolution=16)
    assert big["counts"][0] > 0
    assert vsctx.cloud_poisson(p, N, resolution=16, trim=2 * big["density"].max())["counts"].tolist() == [0, 0]
    same = vsctx.cloud_poisson(p, N, resolution=16, density=False)  # vs_cloud_poisson_density with NULL outputs
    assert np.array_equal(same["tri"], big["tri"]) and np.array_equal(bits(same["verts"]), bits(big["verts"]))
    plain = vsctx.cloud_poisson(p, N, resolution=16)
    assert np.array_equal(same["tri"], plain["tri"]) and np.array_equal(bits(same["verts"]), bits(plain["verts"]))
    import torch  # the enqueue-only call cannot return the missing extent: it reports it on the device
    dev = dict(dtype=torch.float64, device="cuda")
    d_p, d_n, verts, vd = torch.ones((5000, 3), **dev), torch.ones((5000, 3), **dev), torch.zeros((64, 3), **dev), torch.zeros(64, **dev)
    tri = torch.zeros((64, 3), dtype=torch.int32, device="cuda")
    cnt, info = torch.full((2,), -7, dtype=torch.int32, device="cuda"), torch.zeros(4, **dev)
    cfg = vsctx.poisson_config(resolution=16, solver=1, point_weight=6.0, trim=1.0)
    vsctx.cloud_poisson_density_dev(d_p.data_ptr(), d_n.data_ptr(), 5000, cfg, 64, 64, verts.data_ptr(), tri.data_ptr(),
                                    cnt.data_ptr(), info.data_ptr(), vd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0] and info.tolist() == [0.0, 0.0, 0.0, -1.0]
