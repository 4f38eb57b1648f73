"""Times the sparse-map cloud filter (vs_cloud_filter_dev) and its k-NN stage alone (vs_cloud_knn_dev)
at the tracking tests' map sizes, with device events over repeated calls after warm-up.

    python tools/bench_cloud.py [--out profiles/cloud_filter.json] [--sizes 12000 60000] [--k 25]
    python tools/bench_cloud.py --densify [--out profiles/cloud_densify.json]

--densify times vs_cloud_normals_dev (k = 20) and vs_cloud_densify_dev with the same protocol on the same cloud with
holes cut into the planes, and a second pass with the context's stage profile on gives each kernel's share.
    python tools/bench_cloud.py --grid [--out profiles/cloud_knn_grid.json]

--grid times the cell-grid entry points (vs_cloud_knn_grid_dev, vs_cloud_normals_grid_dev with k = 20,
vs_cloud_filter_grid_dev) beside their brute-force counterparts in the same run, then alone at 2^20 points, and
reports the stats pair and each kernel's share and time per launch from a profile pass of its own.
    python tools/bench_cloud.py --mesh [--out profiles/cloud_mesh.json]

--mesh times vs_cloud_mesh_dev on --densify's cloud with precomputed normals, brute force and grid, then on the grid
at 2^20 points, beside vs_cloud_normals[_grid]_dev at the same n, and each kernel's share from a profile pass.

    python tools/bench_cloud.py --poisson [--out profiles/cloud_poisson.json]

--poisson times vs_cloud_poisson_dev (normals precomputed with k = 20 and oriented towards a view inside the room) on
--densify's cloud without its far outliers at R = 64, 128, 256 (--resolutions), and reports the conjugate-gradient
iterations and, from a profile pass of its own, each kernel's share and time per launch and the solve's own time (the
k_cg_* or k_dst_* kernels).  --solver direct selects the sine-transform solve (csrc/poisson_dst.hip); its passes are
then set against the card's peaks: a pass moves 16 R^3 bytes and does 2 R^4 flop (the z pair twice that), against
8 TB/s of HBM and 78.6 TFLOP/s of fp64 matrix arithmetic.  --point-weight adds the screened solve (step 4s): its
iterations, and from the profile pass (run with max_iter = the measured count under the preconditioner, so that no
idle launch is averaged in) the time per iteration of the operator (k_sc_apply), the interpolation (k_sc_interp), the
preconditioner (k_dst_*) and the updates (k_sc_update, k_sc_rz).  --trim adds step 7 and times the untrimmed call of
the same settings beside it, rounds alternating.

Pair tests per filter call = n0^2 + n1^2 (n0 points enter statistical_outlier_removal, n1 enter
surface_aware_filter: every query meets every candidate).  One pair test is 3 sub, 3 mul, 2 add and
1 compare in fp64, none of them fused; the fp64 VALU peak used for the share is 78.6 TFLOP/s counting
an FMA as two, i.e. 39.3e12 unfused instructions per second per lane-op."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-slam-pipeline_amd", "python"))
import vslam_abi  # noqa: E402

PEAK_FP64_OPS = 39.3e12  # unfused fp64 VALU instructions (lane-ops) per second, MI355X
OPS_PER_PAIR = 9


def cloud(n, seed=1):
    """Two noisy planes, a volumetric blob and 2 % far outliers (the shape of a sparse indoor map)."""
    rng = np.random.default_rng(seed)
    n_out, n_pl = n // 50, (n - n // 50) * 3 // 8
    uv = rng.uniform(0, 4, (2, n_pl, 2))
    a = np.column_stack([uv[0], 0.002 * rng.standard_normal(n_pl)])
    b = np.column_stack([0.002 * rng.standard_normal(n_pl) + 4.5, uv[1]])
    blob = rng.uniform(0, 1.5, (n - n_out - 2 * n_pl, 3)) + [1.0, 4.5, 1.0]
    return rng.permutation(np.concatenate([a, b, blob, rng.uniform(-12, 12, (n_out, 3))]))


def holed(p):
    """The cloud without the points of a 0.5 m lattice of discs (radius 0.1 m) on either plane."""
    def disc(u, v):
        return np.hypot((u + 0.25) % 0.5 - 0.25, (v + 0.25) % 0.5 - 0.25) < 0.1
    on_a, on_b = np.abs(p[:, 2]) < 0.02, np.abs(p[:, 0] - 4.5) < 0.02
    return p[~((on_a & disc(p[:, 0], p[:, 1])) | (on_b & disc(p[:, 1], p[:, 2])))]


def densify_runs(ctx, sizes, stream, dev):
    s, runs = stream.cuda_stream, []
    for n0 in sizes:
        p = torch.from_numpy(np.ascontiguousarray(holed(cloud(n0)))).to(dev)
        n, cap = p.shape[0], p.shape[0] * 26
        nrm = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        out = torch.zeros((cap, 3), dtype=torch.float64, device=dev)
        src = torch.zeros(cap, dtype=torch.int32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        reps = max(10, int(5e9 / (n * n)))
        normals = lambda: ctx.cloud_normals_dev(p.data_ptr(), n, 20, nrm.data_ptr(), None, s)  # noqa: E731
        densify = lambda: ctx.cloud_densify_dev(p.data_ptr(), n, None, cap, out.data_ptr(), src.data_ptr(),  # noqa: E731
                                                cnt.data_ptr(), s)
        n_ms, d_ms = timed(normals, stream, 5, reps), timed(densify, stream, 5, reps)
        ctx.profile(True)  # a pass of its own: the stage events are not part of the timed calls above
        ctx.profile_reset()
        for _ in range(10):
            densify()
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        ctx.profile(False)
        tot = sum(ms for ms, _ in prof.values()) or 1.0
        runs.append({"n_before_holes": n0, "n": n, "counts": cnt.cpu().numpy().tolist(), "reps_per_round": reps,
                     "normals_ms_rounds": n_ms, "normals_ms": float(np.median(n_ms)),
                     "densify_ms_rounds": d_ms, "densify_ms": float(np.median(d_ms)),
                     "densify_kernel_share": {k: ms / tot for k, (ms, _) in prof.items()}})
    return runs


def grid_runs(ctx, args, cfg, stream, dev):
    s, runs = stream.cuda_stream, []
    for n in args.sizes + [1 << 20]:
        brute = n <= (1 << 18)
        p = torch.from_numpy(cloud(n)).to(dev)
        out = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        idx = torch.zeros(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(3, dtype=torch.int32, device=dev)
        nbr = torch.zeros((n, args.k), dtype=torch.int32, device=dev)
        d2 = torch.zeros((n, args.k), dtype=torch.float64, device=dev)
        stats = torch.zeros(2, dtype=torch.int32, device=dev)
        calls = {
            "knn": lambda g: (ctx.cloud_knn_grid_dev(p.data_ptr(), n, args.k, nbr.data_ptr(), d2.data_ptr(), 0.0, 0,
                                                     stats.data_ptr(), s) if g else
                              ctx.cloud_knn_dev(p.data_ptr(), n, args.k, nbr.data_ptr(), d2.data_ptr(), 0, s)),
            "normals": lambda g: ctx.cloud_normals_dev(p.data_ptr(), n, 20, out.data_ptr(), None, s, grid=g),
            "filter": lambda g: ctx.cloud_filter_dev(p.data_ptr(), n, cfg, out.data_ptr(), idx.data_ptr(),
                                                     cnt.data_ptr(), s, grid=g),
        }
        run = {"n": n, "reps_per_round": {}}
        for name, call in calls.items():
            for g in ([False, True] if brute else [True]):
                reps = max(3, min(100, int((2e7 if g else 2e10 / n) / n)))
                ms = timed(lambda: call(g), stream, 5, reps)
                key = name + ("_grid" if g else "")
                run[key + "_ms_rounds"], run[key + "_ms"] = ms, float(np.median(ms))
                run["reps_per_round"][key] = reps
            if brute:
                run[name + "_brute_over_grid"] = run[name + "_ms"] / run[name + "_grid_ms"]
        run["stats"] = stats.cpu().numpy().tolist()
        run["filter_counts"] = cnt.cpu().numpy().tolist()
        ctx.profile(True)  # a pass of its own: the stage events are not part of the timed calls above
        ctx.profile_reset()
        for _ in range(5):
            calls["knn"](True)
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        ctx.profile(False)
        tot = sum(ms for ms, _ in prof.values()) or 1.0
        run["knn_grid_kernel_share"] = {k: ms / tot for k, (ms, _) in prof.items()}
        run["knn_grid_kernel_ms_per_launch"] = {k: ms / max(c, 1) for k, (ms, c) in prof.items()}
        runs.append(run)
    return runs


def mesh_runs(ctx, sizes, stream, dev):
    s, runs = stream.cuda_stream, []
    for n0 in sizes + [1 << 20]:
        p = torch.from_numpy(np.ascontiguousarray(holed(cloud(n0)))).to(dev)
        n, cap = p.shape[0], p.shape[0] * 19
        nrm = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        scratch = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        tri = torch.zeros((cap, 3), dtype=torch.int32, device=dev)
        cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        run = {"n_before_holes": n0, "n": n, "reps_per_round": {}}
        for g in ([False, True] if n <= (1 << 18) else [True]):
            cfg = ctx.mesh_config(grid=g)
            ctx.cloud_normals_dev(p.data_ptr(), n, 20, nrm.data_ptr(), None, s, grid=g)  # precomputed: not timed
            mesh = lambda: ctx.cloud_mesh_dev(p.data_ptr(), nrm.data_ptr(), n, cfg, cap, tri.data_ptr(),  # noqa: E731
                                              cnt.data_ptr(), s)
            normals = lambda: ctx.cloud_normals_dev(p.data_ptr(), n, 20, scratch.data_ptr(), None, s, grid=g)  # noqa: E731
            reps = max(3, min(100, int((2e7 if g else 2e10 / n) / n)))
            key = "_grid" if g else ""
            for name, call in (("mesh", mesh), ("normals", normals)):
                ms = timed(call, stream, 5, reps)
                run[name + key + "_ms_rounds"], run[name + key + "_ms"] = ms, float(np.median(ms))
            run["reps_per_round"]["mesh" + key] = reps
            ctx.profile(True)  # a pass of its own: the stage events are not part of the timed calls above
            ctx.profile_reset()
            for _ in range(5):
                mesh()
            torch.cuda.synchronize()
            prof = {k: v for k, v in ctx.profile_read().items() if v[1] > 0}  # the stages this path launched
            ctx.profile(False)
            tot = sum(ms for ms, _ in prof.values()) or 1.0
            run["mesh" + key + "_kernel_share"] = {k: ms / tot for k, (ms, _) in prof.items()}
            run["mesh" + key + "_kernel_ms_per_launch"] = {k: ms / max(c, 1) for k, (ms, c) in prof.items()}
            run["counts" + key] = cnt.cpu().numpy().tolist()
        runs.append(run)
    return runs


PEAK_HBM, PEAK_FP64_MATRIX = 8.0e12, 78.6e12


def poisson_runs(ctx, sizes, stream, dev, solver, resolutions, point_weight=0.0, trim=0.0, max_iter=0):
    s, runs = stream.cuda_stream, []
    p = holed(cloud(sizes[-1]))
    p = torch.from_numpy(np.ascontiguousarray(p[np.all(np.abs(p - 2.5) < 4.0, axis=1)])).to(dev)  # the room alone
    n, vcap, tcap = p.shape[0], 1 << 22, 1 << 23
    nrm = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    view = torch.tensor([[2.0, 2.0, 2.0]], dtype=torch.float64, device=dev)
    verts = torch.zeros((vcap, 3), dtype=torch.float64, device=dev)
    tri = torch.zeros((tcap, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.float64, device=dev)
    ctx.cloud_normals_dev(p.data_ptr(), n, 20, nrm.data_ptr(), None, s)
    ctx.cloud_orient_normals_dev(p.data_ptr(), nrm.data_ptr(), n, view.data_ptr(), 1, s)
    for R in resolutions:
        extra = {"point_weight": point_weight, "trim": trim} if point_weight or trim else {}  # the plain call: the config as it was
        base = dict(resolution=R, solver=1 if solver == "direct" else 0, **({"point_weight": point_weight} if point_weight else {}),
                    **({"max_iter": max_iter} if max_iter else {}))
        enqueue = lambda c: ctx.cloud_poisson_dev(p.data_ptr(), nrm.data_ptr(), n, c, vcap, tcap, verts.data_ptr(),  # noqa: E731
                                                  tri.data_ptr(), cnt.data_ptr(), info.data_ptr(), s)
        cfg = ctx.poisson_config(**base, **({"trim": trim} if trim else {}))
        call = lambda: enqueue(cfg)  # noqa: E731
        reps = 2 if R > 128 else 5
        if trim:  # the untrimmed call of the same session, its rounds between the trimmed call's
            untrimmed = ctx.poisson_config(**base)
            pairs = [(timed(call, stream, 1, reps, 1)[0], timed(lambda: enqueue(untrimmed), stream, 1, reps, 1)[0]) for _ in range(5)]
            ms, extra["untrimmed_ms_rounds"] = [a for a, _ in pairs], [b for _, b in pairs]
            extra["untrimmed_ms"] = float(np.median(extra["untrimmed_ms_rounds"]))
            call()
        else:
            ms = timed(call, stream, 1, reps)
        torch.cuda.synchronize()
        it = info.cpu().numpy().tolist()
        if point_weight and solver == "direct":
            cfg = ctx.poisson_config(**{**base, "max_iter": max(int(it[0]), 1)}, **({"trim": trim} if trim else {}))
        ctx.profile(True)  # a pass of its own: the stage events are not part of the timed calls above
        ctx.profile_reset()
        call()
        torch.cuda.synchronize()
        prof = {k: v for k, v in ctx.profile_read().items() if v[1] > 0}
        ctx.profile(False)
        tot = sum(v[0] for v in prof.values()) or 1.0
        solve = {k: v for k, v in prof.items() if k.startswith(("k_cg_", "k_dst_", "k_sc_"))}
        run = {"solver": solver, "solve_ms": sum(v[0] for v in solve.values()), **extra}
        if point_weight:
            group = lambda *names: sum(v[0] for k, v in prof.items() if k.startswith(names))  # noqa: E731
            its = max(int(it[0]), 1)
            run["screened_ms_per_iteration"] = {
                "apply": group("k_sc_apply") / (its + 1), "interp": group("k_sc_interp") / (its + 1),
                "preconditioner": group("k_dst_") / (its + 2) if solver == "direct" else 0.0,
                "updates": group("k_sc_update", "k_sc_rz") / its}
        if solver == "direct":  # per transform pass: the z pair is one launch of two products
            run["passes"] = {}
            for k, v in solve.items():
                if k in ("k_dst_i", "k_dst_j", "k_dst_z", "k_dst_zz"):
                    sec, flop = v[0] / v[1] * 1e-3, (4.0 if k == "k_dst_zz" else 2.0) * R ** 4
                    run["passes"][k] = {"ms_per_launch": v[0] / v[1], "tb_per_s": 16.0 * R ** 3 / sec / 1e12,
                                        "tflop_per_s": flop / sec / 1e12,
                                        "share_of_hbm_peak": 16.0 * R ** 3 / sec / PEAK_HBM,
                                        "share_of_fp64_matrix_peak": flop / sec / PEAK_FP64_MATRIX}
        runs.append({**run, "n": n, "resolution": R, "reps_per_round": reps, "poisson_ms_rounds": ms,
                     "poisson_ms": float(np.median(ms)), "iterations": int(it[0]), "relative_residual": it[1],
                     "iso": it[2], "converged": int(it[3]), "iterations_enqueued": 0 if solver == "direct" else 8 * R,
                     "counts": cnt.cpu().numpy().tolist(),
                     "kernel_share": {k: v[0] / tot for k, v in prof.items()},
                     "kernel_ms_total": {k: v[0] for k, v in prof.items()},
                     "kernel_launches": {k: v[1] for k, v in prof.items()}})
    return runs


def timed(fn, stream, warm, reps, rounds=5):
    """ms per call: events on the stream the calls are enqueued on, around reps calls, per round."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[12000, 60000])
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--densify", action="store_true")
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--poisson", action="store_true")
    ap.add_argument("--solver", choices=["cg", "direct"], default="cg")
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--point-weight", type=float, default=0.0)
    ap.add_argument("--trim", type=float, default=0.0)
    ap.add_argument("--max-iter", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "cus": cus, "k": args.k, "runs": []}
    with vslam_abi.Context(0) as ctx:
        cfg = ctx.cloud_config(sor_k=args.k, surf_k=args.k)
        stream = torch.cuda.ExternalStream(ctx.stream)  # the context's own stream
        if args.densify:
            res = {"device": res["device"], "cus": cus, "runs": densify_runs(ctx, args.sizes, stream, dev)}
        elif args.grid:
            res["runs"] = grid_runs(ctx, args, cfg, stream, dev)
        elif args.poisson:
            res = {"device": res["device"], "cus": cus, "runs": poisson_runs(ctx, args.sizes, stream, dev, args.solver, args.resolutions,
                                                                             args.point_weight, args.trim, args.max_iter)}
        elif args.mesh:
            res = {"device": res["device"], "cus": cus, "runs": mesh_runs(ctx, args.sizes, stream, dev)}
        else:
            res["runs"] = filter_runs(ctx, args, cfg, cus, stream, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def filter_runs(ctx, args, cfg, cus, stream, dev):
    s, runs = stream.cuda_stream, []
    for n in args.sizes:
        p = torch.from_numpy(cloud(n)).to(dev)
        out = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        idx = torch.zeros(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(3, dtype=torch.int32, device=dev)
        nbr = torch.zeros((n, args.k), dtype=torch.int32, device=dev)
        d2 = torch.zeros((n, args.k), dtype=torch.float64, device=dev)
        reps = max(10, int(2e10 / (n * n)))
        f_ms = timed(lambda: ctx.cloud_filter_dev(p.data_ptr(), n, cfg, out.data_ptr(), idx.data_ptr(),
                                                  cnt.data_ptr(), s), stream, 5, reps)
        k_ms = timed(lambda: ctx.cloud_knn_dev(p.data_ptr(), n, args.k, nbr.data_ptr(), d2.data_ptr(), 0, s),
                     stream, 5, reps)
        c = cnt.cpu().numpy().tolist()
        blocks = (n + 255) // 256
        split = max(1, min(-(-cus // blocks), n // 512, 64))  # cloud.hip knn_split
        pairs_f, pairs_k = float(c[0]) ** 2 + float(c[1]) ** 2, float(n) ** 2
        run = {"n": n, "counts": c, "split": split, "reps_per_round": reps,
               "filter_ms_rounds": f_ms, "filter_ms": float(np.median(f_ms)),
               "knn_ms_rounds": k_ms, "knn_ms": float(np.median(k_ms))}
        run["filter_pair_tests_per_s"] = pairs_f / (run["filter_ms"] * 1e-3)
        run["knn_pair_tests_per_s"] = pairs_k / (run["knn_ms"] * 1e-3)
        run["filter_share_of_fp64_valu_peak"] = run["filter_pair_tests_per_s"] * OPS_PER_PAIR / PEAK_FP64_OPS
        run["knn_share_of_fp64_valu_peak"] = run["knn_pair_tests_per_s"] * OPS_PER_PAIR / PEAK_FP64_OPS
        runs.append(run)
    return runs


if __name__ == "__main__":
    main()
