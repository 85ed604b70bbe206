"""mi_skin_frame against what a caller does today for the same results, on one box.

    python tools/probes/skinning_probe.py [--scenes foxes,humanoids] [--reps 15] [--out FILE.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/probes/skinning_probe.py --trace-only     (kernel time, a run of its own)

Scenes: foxes = 1 000 skins x 24 joints x 24 joint AABBs; humanoids = 14 706 rigs x 68 joints x 68 joint AABBs (~1 M slots).  Joints
and meshes are rows of one context; their GlobalTransforms are uploaded once (rotation x scale x translation, well conditioned).
  device    mi_skin_frame (matrices + bounds) alone: events around enough back-to-back calls to fill ~0.2 s, per call
  dev+dl    mi_skin_frame + mi_skin_download_matrices + mi_skin_download_bounds, wall clock
  dev+cull  mi_skin_frame + mi_cull + synchronize, wall clock: the frame stays on the device
  host      mi_download_global_transforms + the numpy product and refit (f32, vectorised over all skins) + mi_upload_bounds +
            mi_cull + synchronize (the cull pays the row-summary rebuild the upload triggers), wall clock
The wall-clock figures alternate in one loop; median and the quartile range over --reps rounds.
Bytes the kernel needs (an estimate from the shapes, not a counter): 200 per slot -- 8 of indices, 64 of bindpose, up to two 64-byte
lines for the gathered 48-byte row, 64 out -- and 100 per joint AABB -- 4 + 24 of box, 4 of row index, the row's lines."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bevy_amd as B  # noqa: E402

F32, U32 = np.float32, np.uint32
SCENES = {"foxes": (1000, 24), "humanoids": (14706, 68)}
BYTES_PER_SLOT, BYTES_PER_AABB = 200, 100


def m3v(m, v):
    return (m[..., 0, :] * v[..., 0:1] + m[..., 1, :] * v[..., 1:2]) + m[..., 2, :] * v[..., 2:3]


def host_skinning(g, n_skins, k, pool, a_c, a_h):
    """What extract_skins and update_skinned_mesh_bounds compute, f32, for n_skins skins of k joints (slots first, meshes behind),
    AABB j of a skin on its joint j.  -> matrices [n_skins k, 16], centre and half extents [n_skins, 3]"""
    gj = g[:n_skins * k].reshape(-1, 4, 3)
    axes = np.zeros((len(gj), 4, 4), F32)
    axes[:, :, :3] = gj
    axes[:, 3, 3] = 1
    b = np.tile(pool.reshape(-1, 4, 4), (n_skins, 1, 1))
    mats = np.empty_like(b)
    for c in range(4):
        mats[:, c] = ((axes[:, 0] * b[:, c, 0:1] + axes[:, 1] * b[:, c, 1:2]) + axes[:, 2] * b[:, c, 2:3]) + axes[:, 3] * b[:, c, 3:4]
    x, y, z, t = (g[n_skins * k:].reshape(-1, 4, 3)[:, i] for i in range(4))
    t2 = np.cross(x, y)
    inv = (F32(1) / ((z * t2).sum(1, dtype=F32)))[:, None]
    em = np.stack([np.cross(y, z) * inv, np.cross(z, x) * inv, t2 * inv], axis=2)[:, None]  # [skin, 1, column, row]
    et = -m3v(em[:, 0], t)
    gs = gj.reshape(n_skins, k, 4, 3)
    am = np.stack([m3v(em, gs[:, :, i]) for i in range(3)], axis=2)
    cc = m3v(am, a_c.reshape(n_skins, k, 3)) + (m3v(em, gs[:, :, 3]) + et[:, None])
    hh = m3v(np.abs(am), a_h.reshape(n_skins, k, 3))
    lo, hi = (cc - hh).min(1), (cc + hh).max(1)
    return mats.reshape(-1, 16), (hi + lo) * F32(0.5), (hi - lo) * F32(0.5)


def setup(ctx, name):
    n_skins, k = SCENES[name]
    rng = np.random.default_rng(n_skins)
    n_slots, n = n_skins * k, n_skins * k + n_skins
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y), 2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x),
                    2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3) * rng.uniform(0.5, 2, (n, 3, 1))
    g = np.concatenate([rot.reshape(n, 9), rng.uniform(-100, 100, (n, 3))], axis=1).astype(F32)
    pool = rng.normal(size=(k, 16)).astype(F32)
    a_c, a_h = rng.normal(size=(n_slots, 3)).astype(F32), rng.uniform(0.1, 1, (n_slots, 3)).astype(F32)
    skins = np.array([[n_slots + i, i * k, k, 0, i * k, k] for i in range(n_skins)], U32)
    ctx.resize(n)
    ctx.upload_global_transforms(g.reshape(-1))
    ctx.upload_bounds(np.zeros(3 * n, F32), np.ones(3 * n, F32))
    ctx.upload_inverse_bindposes(pool)
    ctx.upload_skins(skins, np.arange(n_slots, dtype=U32), np.tile(np.arange(k, dtype=U32), n_skins), a_c, a_h)
    return n_skins, k, g, pool, a_c, a_h


def run(name, reps):
    frustum = np.tile(np.array([0, 0, 0, 1], F32), 6)
    whole = B.CULL_BEGIN_FRAME | B.CULL_END_FRAME
    with B.Context() as ctx:
        n_skins, k, g, pool, a_c, a_h = setup(ctx, name)
        n_slots, n = n_skins * k, n_skins * k + n_skins

        def device(calls):
            ctx.timer_begin()
            for _ in range(calls):
                ctx.skin_frame()
            return 1e3 * ctx.timer_end() / calls

        def dev_dl():
            t0 = time.perf_counter()
            ctx.skin_frame()
            dev_dl.m, dev_dl.b = ctx.download_joint_matrices(), ctx.download_skin_bounds()
            return 1e6 * (time.perf_counter() - t0)

        def dev_cull():
            t0 = time.perf_counter()
            ctx.skin_frame()
            ctx.cull(frustum, flags=whole)
            ctx.synchronize()
            return 1e6 * (time.perf_counter() - t0)

        def host():
            t0 = time.perf_counter()
            gh = ctx.download_global_transforms(want_changed=False).reshape(n, 12)
            host.m, c, h = host_skinning(gh, n_skins, k, pool, a_c, a_h)
            host.b = (c, h)
            ctx.upload_bounds(c.reshape(-1), h.reshape(-1), first_row=n_slots)
            ctx.cull(frustum, flags=whole)
            ctx.synchronize()
            return 1e6 * (time.perf_counter() - t0)

        for fn in (dev_dl, dev_cull, host):  # warm-up
            for _ in range(3):
                fn()
        calls = max(10, int(0.2e6 / device(20)))
        dev = [device(calls) for _ in range(5)]
        wall = {fn.__name__: [] for fn in (dev_dl, dev_cull, host)}
        for _ in range(reps):
            for fn in (dev_dl, dev_cull, host):
                wall[fn.__name__].append(fn())
        assert np.array_equal(dev_dl.m.view(U32), host.m.view(U32))
        # (the refit's min / max order does not matter, but numpy's cross product associates as glam's: equal bits expected)
        same_bounds = all(np.array_equal(a.view(U32), b.view(U32)) for a, b in zip(dev_dl.b, host.b))
    stat = lambda v: (float(np.median(v)), float(np.percentile(v, 75) - np.percentile(v, 25)))
    return dict(name=name, n_skins=n_skins, k=k, calls=calls, device=stat(dev), same_bounds=same_bounds, **{a: stat(v) for a, v in wall.items()})


def trace_only():
    """Frames for a rocprofv3 --kernel-trace --stats run: 200 launches of k_skin_frame per scene, nothing timed here."""
    for name in SCENES:
        with B.Context() as ctx:
            setup(ctx, name)
            for _ in range(200):
                ctx.skin_frame()
            ctx.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="foxes,humanoids")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.trace_only:
        return trace_only()
    lines = ["| scene | slots | mi_skin_frame (device, µs; calls per window) | GB/s by the byte estimate | + both downloads (wall, µs) | + cull, no download (wall, µs) | host path + cull (wall, µs) | bounds bit-equal to numpy |",
             "|---|---|---|---|---|---|---|---|"]
    pm = lambda s: f"{s[0]:.0f} ± {s[1]:.0f}"
    for name in a.scenes.split(","):
        r = run(name, a.reps)
        slots = r["n_skins"] * r["k"]
        nbytes = BYTES_PER_SLOT * slots + BYTES_PER_AABB * slots
        lines.append(f"| {name}: {r['n_skins']} x {r['k']} | {slots} | {r['device'][0]:.1f} ± {r['device'][1]:.1f} ({r['calls']}) | {nbytes / r['device'][0] * 1e-3:.0f} | "
                     f"{pm(r['dev_dl'])} | {pm(r['dev_cull'])} | {pm(r['host'])} | {r['same_bounds']} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
