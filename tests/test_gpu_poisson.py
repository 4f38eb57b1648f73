"""Poisson surface reconstruction on the GPU (csrc/cloud_poisson.hip) against a plain numpy fp64 restatement of the
semantics in include/vslam_abi.h: np.add.at for the splat, the discrete sine transform for the solve (it shares nothing
with conjugate gradients), Python loops over the tetrahedra.  Where a decision hangs on field < iso the restatement
asserts on its own data that no node lies near iso; the seeds were checked on the CPU."""
import functools

import numpy as np
import pytest

import vslam_abi

pytestmark = pytest.mark.gpu

KINDS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def at(F, q):
    """Field values at integer nodes q [..., 3] = (i, j, k); the field is indexed [k, j, i]."""
    return F[q[..., 2], q[..., 1], q[..., 0]]


def ref_grid(p, R, scale=1.1):
    lo, hi = p.min(0), p.max(0)
    side = scale * (hi - lo).max()
    return (lo + hi) / 2 - side / 2, side / (R - 1)


def ref_trilinear(p, o, h, R):
    """-> per point the 8 nodes [n, 8, 3] and weights [n, 8], offsets in the order dx + 2 dy + 4 dz."""
    g = (p - o) / h
    b = np.clip(np.floor(g).astype(np.int64), 0, R - 2)
    f = g - b
    d = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])
    w = np.where(d[None] == 1, f[:, None, :], 1.0 - f[:, None, :])
    return b[:, None, :] + d[None], (w[..., 0] * w[..., 1]) * w[..., 2]


def ref_rhs(p, N, R):
    o, h = ref_grid(p, R)
    q, w = ref_trilinear(p, o, h, R)
    V = np.zeros((3, R + 2, R + 2, R + 2))  # one node of zeros around the grid
    for ax in range(3):
        np.add.at(V[ax], (q[..., 2] + 1, q[..., 1] + 1, q[..., 0] + 1), w * N[:, None, ax])
    c = slice(1, -1)
    return ((V[0][c, c, 2:] - V[0][c, c, :-2]) + (V[1][c, 2:, c] - V[1][c, :-2, c]) + (V[2][2:, c, c] - V[2][:-2, c, c])) / (2 * h)


def ref_solve(div, h):
    """A chi = -div by the sine transform -> (chi, cond(A))."""
    R = div.shape[0]
    m = np.arange(1, R + 1)
    S = np.sin(np.pi * np.outer(m, m) / (R + 1))
    ev = 1.0 - np.cos(np.pi * m / (R + 1))
    lam = (2.0 / (h * h)) * (ev[:, None, None] + ev[None, :, None] + ev[None, None, :])
    T = np.einsum("ck,bj,ai,kji->cba", S, S, S, -div, optimize=True) / lam
    return np.einsum("ck,bj,ai,cba->kji", S, S, S, T, optimize=True) * (2.0 / (R + 1)) ** 3, lam.max() / lam.min()


def ref_iso_value(chi, p, o, h):
    q, w = ref_trilinear(p, o, h, chi.shape[0])
    return (w * at(chi, q)).sum(1).mean()


def ref_isosurface(F, o, h, iso, band):
    """-> (verts [V, 3], tri [T, 3]) in the order of vslam_abi.h step 6."""
    R = F.shape[0]
    assert np.abs(F - iso).min() >= band, "a node lies in the band around iso: pick another field or seed"
    below = F < iso
    keys = []
    for kind, (dx, dy, dz) in enumerate(KINDS):
        k, j, i = np.nonzero(below[:R - dz, :R - dy, :R - dx] != below[dz:, dy:, dx:])
        keys.append(7 * ((k * R + j) * R + i) + kind)
    keys = np.sort(np.concatenate(keys))
    a = np.stack([keys // 7 % R, keys // 7 // R % R, keys // 7 // (R * R)], 1)
    b = a + np.array(KINDS)[keys % 7]
    t = (iso - at(F, a)) / (at(F, b) - at(F, a))
    pa, pb = o + h * a, o + h * b
    verts = pa + t[:, None] * (pb - pa)
    lin = lambda q: (q[2] * R + q[1]) * R + q[0]  # noqa: E731
    vid = lambda e: int(np.searchsorted(keys, 7 * lin(e[0]) + KINDS.index(tuple(e[1] - e[0]))))  # noqa: E731
    n_below = sum(below[dz:R - 1 + dz, dy:R - 1 + dy, dx:R - 1 + dx].astype(int) for dx, dy, dz in KINDS + [(0, 0, 0)])
    tri = []
    for k, j, i in zip(*np.nonzero((n_below > 0) & (n_below < 8))):  # cubes in linear order
        for perm in PERMS:
            v = [np.array([i, j, k])]
            for ax in perm:
                v.append(v[-1] + np.eye(3, dtype=np.int64)[ax])
            lo = [s for s in range(4) if at(below, v[s])]
            hi = [s for s in range(4) if s not in lo]
            if not lo or not hi:
                continue
            D = len(lo) * sum(v[s] for s in hi) - len(hi) * sum(v[s] for s in lo)
            edge = lambda s, u: (v[min(s, u)], v[max(s, u)])  # noqa: E731
            if len(lo) == 2:
                q = [edge(lo[0], hi[0]), edge(lo[0], hi[1]), edge(lo[1], hi[1]), edge(lo[1], hi[0])]
                cand = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
            else:
                s = lo[0] if len(lo) == 1 else hi[0]
                cand = [[edge(s, u) for u in range(4) if u != s]]
            for es in cand:
                m, ids = [e[0] + e[1] for e in es], [vid(e) for e in es]
                if not np.dot(np.cross(m[1] - m[0], m[2] - m[0]), D) > 0:
                    ids[1], ids[2] = ids[2], ids[1]
                f = int(np.argmin(ids))
                tri.append(ids[f:] + ids[:f])
    return verts, np.array(tri, np.int32).reshape(-1, 3)


def closed(tri):
    """Every directed edge occurs once and its reverse occurs once: a closed oriented manifold."""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
    fwd, rev = e[:, 0] << 32 | e[:, 1], e[:, 1] << 32 | e[:, 0]
    return len(tri) > 0 and len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


@functools.lru_cache(maxsize=None)
def slab(R):
    """A slab of points with random unit normals, the box's corners among them and one point exactly on a node
    -> (points, normals, reference div, h)."""
    rng = np.random.default_rng(R)
    p = np.concatenate([[[0, 0, 0], [1, 1, 0.3]], rng.uniform(0, 1, (300, 3)) * [1, 1, 0.3]])
    o, h = ref_grid(p, R)
    # per axis the first node m inside the box with a coordinate c that gives g = (c - o) / h == m exactly
    node = [next(c for m in range(R) for c in (o[ax] + h * m, np.nextafter(o[ax] + h * m, 9), np.nextafter(o[ax] + h * m, -9))
                 if (c - o[ax]) / h == m and 0 < c < p[1, ax]) for ax in range(3)]
    p = np.concatenate([p, [node]])
    g = (p[-1] - o) / h
    assert np.array_equal(g, np.floor(g)) and np.array_equal(ref_grid(p, R)[0], o)
    N = rng.standard_normal((len(p), 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return p, N, ref_rhs(p, N, R), h


@pytest.mark.parametrize("R", [16, 21, 65])  # 65: a cell index of more than 18 bits, the point sort's third pass
def test_rhs(vsctx, R):
    p, N, div, _ = slab(R)
    runs = [vsctx.cloud_poisson(p, N, fields=True, resolution=R, max_iter=1)["rhs"] for _ in range(2)]
    err = np.abs(runs[0] - div).max() / np.abs(div).max()
    print("R", R, "rhs error / max|rhs|", err)
    assert err <= 1e-12
    assert np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))


@pytest.mark.parametrize("R", [16, 21, 33])
def test_solve(vsctx, R):
    p, N = slab(16)[:2]
    div = ref_rhs(p, N, R)
    chi, cond = ref_solve(div, ref_grid(p, R)[1])
    runs = [vsctx.cloud_poisson(p, N, fields=True, resolution=R, tol=1e-12, max_iter=4000) for _ in range(2)]
    err = np.linalg.norm(runs[0]["chi"] - chi) / np.linalg.norm(chi)
    print("R", R, "cond", cond, "iterations", runs[0]["info"][0], "error", err, "bound", 10 * cond * 1e-12)
    assert err <= 10 * cond * 1e-12
    assert runs[0]["info"][3] == 1 and 0 < runs[0]["info"][0] < 4000 and runs[0]["info"][1] <= 1e-12
    assert runs[0]["info"][0] == runs[1]["info"][0]
    assert np.array_equal(runs[0]["chi"].view(np.uint64), runs[1]["chi"].view(np.uint64))
    short = vsctx.cloud_poisson(p, N, resolution=R, tol=1e-12, max_iter=3)["info"]
    assert short[0] == 3 and short[3] == 0


@functools.lru_cache(maxsize=None)
def bumpy(R):
    """Distance to an off-centre point minus a radius plus a small sinusoid -> (field, origin, h, iso, verts, tri)."""
    h, o = 2.0 / (R - 1), np.array([-1.0, -1.0, -1.0])
    z, y, x = np.meshgrid(*[o[0] + h * np.arange(R)] * 3, indexing="ij")
    F = np.sqrt((x - 0.13) ** 2 + (y + 0.07) ** 2 + (z - 0.21) ** 2) - 0.55 + 0.08 * np.sin(9 * x) * np.sin(7 * y + 1) * np.sin(8 * z)
    return (F, o, h, 0.01) + ref_isosurface(F, o, h, 0.01, 1e-9)


@pytest.mark.parametrize("R", [16, 21])
def test_isosurface(vsctx, R):
    F, o, h, iso, rverts, rtri = bumpy(R)
    assert closed(rtri)
    verts, tri, counts = vsctx.grid_isosurface(F, o, h, iso)
    print("R", R, "counts", counts.tolist(), "reference", [len(rverts), len(rtri)])
    assert counts.tolist() == [len(rverts), len(rtri)] and np.array_equal(tri, rtri)
    assert np.abs(verts - rverts).max() <= 1e-12 * h
    assert closed(tri)
    vcap, tcap = len(rverts) // 2, len(rtri) // 3  # below the totals: the first cap entries, the totals still reported
    verts, tri, counts = vsctx.grid_isosurface(F, o, h, iso, vcap=vcap, tcap=tcap)
    assert counts.tolist() == [len(rverts), len(rtri)] and np.array_equal(tri, rtri[:tcap])
    assert np.abs(verts - rverts[:vcap]).max() <= 1e-12 * h


@functools.lru_cache(maxsize=None)
def shell(R=32, seed=3, n=3000):
    """A noisy sphere shell, normals with random signs, one view inside -> the numpy pipeline's results."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = u * (1.0 + 0.01 * rng.standard_normal((n, 1)))
    N = u * rng.choice([-1.0, 1.0], (n, 1))
    view = np.array([[0.1, 0.0, 0.05]])
    d = view - p
    flip = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2] < 0
    No = np.where(flip[:, None], -N, N)
    o, h = ref_grid(p, R)
    chi = ref_solve(ref_rhs(p, No, R), h)[0]
    iso = ref_iso_value(chi, p, o, h)
    verts, tri = ref_isosurface(chi, o, h, iso, 1e-6 * np.abs(chi).max())
    assert closed(tri)
    return p, N, view, No, o, h, tri, len(verts)


def test_end_to_end(vsctx):
    p, N, view, No, o, h, rtri, rverts = shell()
    assert np.array_equal(vsctx.cloud_orient_normals(p, N, view), No)
    out = vsctx.cloud_poisson(p, N, views=view, fields=True, resolution=32, tol=1e-12, max_iter=4000)
    assert np.array_equal(out["normals"], No) and out["info"][3] == 1
    chi, iso = out["chi"], out["info"][2]
    assert abs(iso - ref_iso_value(chi, p, o, h)) <= 1e-12 * np.abs(chi).max()
    verts, tri = out["verts"], out["tri"]
    print("counts", out["counts"].tolist(), "reference triangles", len(rtri), "iterations", out["info"][0])
    assert out["counts"].tolist() == [rverts, len(rtri)] and np.array_equal(tri, rtri) and len(verts) == rverts
    assert closed(tri)
    a, b, c = verts[tri[:, 0]], verts[tri[:, 1]], verts[tri[:, 2]]
    nearest = np.argmin((((a + b + c) / 3)[:, None, :] - p[None]) ** 2 @ np.ones(3), axis=1)
    assert np.all((np.cross(b - a, c - a) * No[nearest]).sum(1) > 0)
    est = vsctx.cloud_poisson(p, None, views=view, resolution=32)  # the normals estimated (k = 20), then oriented
    used = vsctx.cloud_orient_normals(p, vsctx.cloud_normals(p, 20)[0], view)
    assert np.array_equal(est["normals"], used) and est["info"][3] == 1 and closed(est["tri"])


def test_arguments(vsctx):
    p, N = slab(16)[:2]
    for bad, code in [({"resolution": 15}, "VS_ERR_ARG"), ({"resolution": 513}, "VS_ERR_CAPACITY"), ({"scale": 1.0}, "VS_ERR_ARG")]:
        with pytest.raises(vslam_abi.VSError, match=code):
            vsctx.cloud_poisson(p, N, **bad)
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_ARG"):
        vsctx.cloud_poisson(np.ones((50, 3)), N[:50], resolution=16)  # all points equal: no extent
    with pytest.raises(vslam_abi.VSError, match="VS_ERR_ARG"):
        vsctx.cloud_poisson(p, None, resolution=16)  # normals to be estimated, but no view to orient them by
    out = vsctx.cloud_poisson(p, np.zeros_like(N), fields=True, resolution=16)
    assert out["counts"].tolist() == [0, 0] and out["info"][0] == 0 and not out["chi"].any()
    import torch  # the enqueue-only call cannot return the missing extent: it reports it on the device
    d_p, d_n = torch.ones((5000, 3), dtype=torch.float64, device="cuda"), torch.ones((5000, 3), dtype=torch.float64, device="cuda")
    verts, tri = torch.zeros((64, 3), dtype=torch.float64, device="cuda"), torch.zeros((64, 3), dtype=torch.int32, device="cuda")
    cnt, info = torch.full((2,), -7, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    vsctx.cloud_poisson_dev(d_p.data_ptr(), d_n.data_ptr(), 5000, vsctx.poisson_config(resolution=16), 64, 64, verts.data_ptr(),
                            tri.data_ptr(), cnt.data_ptr(), info.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0] and info.tolist() == [0.0, 0.0, 0.0, -1.0]
