"""profiles/r10_animation/ab.md: mi_anim_frame + mi_propagate against host sampling + mi_upload_transforms_indexed + mi_propagate,
N rigs x 24 joints, one shared clip (linear tracks, 30 keys, one player per rig); and the deviation of a float32 numpy run of the
test's reference from its float64 run on the test's own inputs (no GPU needed for that part: --deviation).
    python tools/probes/animation_probe.py [--deviation] [--rigs 1000,40000] [--reps 30]
profiles/r11_blend/ab.md: --blend, the crossfade scene -- every rig's player with two layers of a shared pair of clips at weights 0.3 /
0.7 through mi_anim_frame_blended, the same with one layer beside mi_anim_frame on identical work, and the host path (numpy sampling
and blending + mi_upload_transforms_indexed); --blend-deviation, the float32 run of test_gpu_anim_blend's reference (no GPU needed).
profiles/r12_graph/ab.md: --graph, (a) a nested graph with an additive clip through mi_anim_frame_graph against its numpy evaluation +
mi_upload_transforms_indexed, (b) a flat two-clip graph through mi_anim_frame_graph against mi_anim_frame_blended on the same work;
--graph-deviation, the float32 run of test_gpu_anim_graph's reference per shape (no GPU needed).
profiles/r13_weights/ab.md: --weights, N rigs with one target of 52 morph weights each through mi_anim_frame_weights, under the seven-node
graph of --graph and under a root CLIP, against (1) numpy evaluation on a core + one hipMemcpy of the result into the device array and
(2) mi_anim_frame_graph over 18 translation-only targets per rig (54 scalars: the same work laid out a lane per target)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bevy_amd as B  # noqa: E402

F32, U32 = np.float32, np.uint32
JOINTS, KEYS = 24, 30


def deviation():
    import test_gpu_animation as T
    worst = {"translation / scale, in units of the bound": 0.0, "rotation, in units of 2^-24": 0.0}
    for n_targets, interp, k, layout in T.CASES:
        rng = np.random.default_rng(1000 * n_targets + 100 * interp + k)
        per = T.build(rng, n_targets, n_targets + 40, interp, k, layout)[4]
        for x in T.SEEKS:
            for tv in per:
                for c in range(3):
                    if tv[c] is None:
                        continue
                    v64, bound = T.sample(*tv[c], c == 1, interp, F32(x))
                    v32 = T.sample(*tv[c], c == 1, interp, F32(x), F32)[0]
                    if np.all(np.asarray(bound) == 0):
                        assert np.array_equal(v32, v64)
                    elif c == 1:
                        worst["rotation, in units of 2^-24"] = max(worst["rotation, in units of 2^-24"], np.max(np.abs(v32 - v64)) / T.E)
                    else:
                        key = "translation / scale, in units of the bound"
                        worst[key] = max(worst[key], np.max(np.abs(v32 - v64) / bound))
    for k, v in worst.items():
        print(f"float32 numpy against float64, test inputs, worst {k}: {v:.2f}")
    # the cases of the search seams, seek-time edges and many players: the float32 run has to stay inside the test's own bounds
    worst = 0.0
    for name, (fn, *args) in T.NEW_CASES.items():
        case = fn(*args)
        cur = [np.zeros((case["n"], w), F32) for w in (3, 4, 3)]
        for seeks in case["seeks"]:
            (w64, bound), (w32, _) = [T.expected(cur, case["targets"], case["per"], seeks, dt=dt) for dt in (np.float64, F32)]
            for c in range(3):
                exact = bound[c] == 0
                assert np.array_equal(w32[c][exact], w64[c][exact]), (name, c)
                ratio = np.max(np.abs(w32[c] - w64[c])[~exact] / bound[c][~exact], initial=0.0)
                assert ratio <= 1, (name, c, ratio)
                worst = max(worst, ratio)
    print(f"float32 numpy against float64, the {len(T.NEW_CASES)} later cases, worst error / bound: {worst:.2f}")


def clip(rng):
    """One clip: 24 joints x (t, r, s) linear tracks over one range of KEYS times."""
    times = np.linspace(0, 1, KEYS).astype(F32)
    tracks, values, n_v = np.zeros(3 * JOINTS, B.ANIM_TRACK_DTYPE), [], 0
    for j in range(JOINTS):
        for c, (comp, w) in enumerate(((B.ANIM_TRANSLATION, 3), (B.ANIM_ROTATION, 4), (B.ANIM_SCALE, 3))):
            v = rng.normal(0, 1, (KEYS, w))
            if c == 1:
                v /= np.linalg.norm(v, axis=1, keepdims=True)
            tracks[3 * j + c] = (0, KEYS, n_v, comp | B.ANIM_LINEAR)
            values.append(v.astype(F32).reshape(-1))
            n_v += v.size
    return tracks, times, np.concatenate(values)


def host_sample(times, vals, x):
    """numpy sampling of the clip for every rig: vals [JOINTS][3] of [KEYS, w]; x [rigs] -> t [rigs * JOINTS, 3], r, s (nlerp-free
    slerp left out: the host path is charged the cheaper lerp + normalize for rotations)"""
    i = np.clip(np.searchsorted(times, x, side="right") - 1, 0, KEYS - 2)
    u = ((x - times[i]) / (times[i + 1] - times[i])).astype(F32)[:, None, None]
    out = []
    for c in range(3):
        v = vals[c]  # [JOINTS, KEYS, w]
        a, b = v[:, i].transpose(1, 0, 2), v[:, i + 1].transpose(1, 0, 2)
        o = a + (b - a) * u
        if c == 1:
            o /= np.linalg.norm(o, axis=2, keepdims=True)
        out.append(o.reshape(-1, o.shape[2]).astype(F32))
    return out


def quartiles(xs):
    q = np.percentile(np.array(xs) * 1e6, [25, 50, 75])
    return f"{q[1]:.1f} us (quartiles {q[0]:.1f} - {q[2]:.1f})"


def ab(rigs, reps):
    rng = np.random.default_rng(rigs)
    tracks, times, values = clip(rng)
    n = rigs * JOINTS
    targets = np.zeros(n, B.ANIM_TARGET_DTYPE)
    targets["row"], targets["player"] = np.arange(n), np.arange(n) // JOINTS
    for c, f in enumerate(("track_t", "track_r", "track_s")):
        targets[f] = 3 * (np.arange(n) % JOINTS) + c
    vals = [np.stack([values[tracks[3 * j + c]["first_value"]:][:KEYS * w].reshape(KEYS, w) for j in range(JOINTS)]) for c, w in enumerate((3, 4, 3))]
    rows = np.arange(n, dtype=U32)
    dev, host, host_sampling = [], [], []
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(np.zeros(3 * n, F32), np.tile(np.array([0, 0, 0, 1], F32), n), np.ones(3 * n, F32))
        ctx.propagate()
        ctx.anim_upload_tracks(tracks, times, values)
        ctx.anim_upload_targets(targets)
        for rep in range(reps + 5):  # (five warm-up frames)
            x = rng.uniform(0.01, 0.99, rigs).astype(F32)
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.anim_frame(x)
            ctx.propagate(0)
            ctx.synchronize()
            t1 = time.perf_counter()
            t, r, s = host_sample(times, vals, x)
            t2 = time.perf_counter()
            ctx.upload_transforms_indexed(rows, t.reshape(-1), r.reshape(-1), s.reshape(-1))
            ctx.propagate(0)
            ctx.synchronize()
            t3 = time.perf_counter()
            if rep >= 5:
                dev.append(t1 - t0), host.append(t3 - t1), host_sampling.append(t2 - t1)
    print(f"{rigs} rigs x {JOINTS} joints, {reps} frames, wall clock around synchronize:")
    print(f"  anim_frame + propagate                                   {quartiles(dev)}")
    print(f"  numpy sampling + upload_transforms_indexed + propagate   {quartiles(host)}  (the sampling alone {quartiles(host_sampling)})")


def blend_deviation():
    import test_gpu_anim_blend as T
    rot, lerp = 0.0, 0.0
    for n, L in T.CASES:
        sc = T.blend_scene(n, L)
        (w64, bound), (w32, _) = [T.expected(sc, sc["cur"], dt) for dt in (np.float64, F32)]
        for c in range(3):
            exact, err = bound[c] == 0, np.abs(w32[c] - w64[c])
            assert np.array_equal(w32[c][exact], w64[c][exact]), (n, L, c)
            if c == 1:
                rot = max(rot, np.max(err[bound[c] == T.ROT_BOUND], initial=0.0) / T.E)
            else:
                lerp = max(lerp, np.max(err[~exact] / bound[c][~exact], initial=0.0))
    print(f"float32 numpy against float64 over the {len(T.CASES)} blend cases: blended rotations worst {rot:.2f} x 2^-24 (the test's bound: "
          f"{T.ROT_BOUND / T.E:.0f}), translation / scale worst error / bound {lerp:.2f}")


def blend_ab(rigs, reps):
    """Two clips over the same 24 joints; a rig's 24 targets share the 24 x 2 bindings with every other rig."""
    rng = np.random.default_rng(rigs)
    clips = [clip(rng) for _ in range(2)]
    tracks = np.concatenate([c[0] for c in clips])
    tracks["first_time"][3 * JOINTS:] += KEYS
    tracks["first_value"][3 * JOINTS:] += len(clips[0][2])
    times, values = np.concatenate([c[1] for c in clips]), np.concatenate([c[2] for c in clips])
    n = rigs * JOINTS
    single = np.zeros(n, B.ANIM_TARGET_DTYPE)
    single["row"], single["player"] = np.arange(n), np.arange(n) // JOINTS
    bindings = np.zeros(2 * JOINTS, B.ANIM_BINDING_DTYPE)
    for c, f in enumerate(("track_t", "track_r", "track_s")):
        single[f] = 3 * (np.arange(n) % JOINTS) + c
        bindings[f] = 3 * JOINTS * (np.arange(2 * JOINTS) % 2) + 3 * (np.arange(2 * JOINTS) // 2) + c
    targets = np.zeros(n, B.ANIM_BLEND_TARGET_DTYPE)
    targets["row"], targets["player"], targets["first_binding"], targets["n_clips"] = np.arange(n), np.arange(n) // JOINTS, 2 * (np.arange(n) % JOINTS), 2
    vals = [[np.stack([c[2][c[0][3 * j + k]["first_value"]:][:KEYS * w].reshape(KEYS, w) for j in range(JOINTS)]) for k, w in enumerate((3, 4, 3))] for c in clips]
    two, one = np.zeros(2 * rigs, B.ANIM_LAYER_DTYPE), np.zeros(rigs, B.ANIM_LAYER_DTYPE)
    two["player"], two["clip"], two["weight"] = np.arange(2 * rigs) // 2, np.arange(2 * rigs) % 2, np.tile(np.array([0.3, 0.7], F32), rigs)
    one["player"], one["weight"] = np.arange(rigs), 1.0
    rows = np.arange(n, dtype=U32)
    took = {k: [] for k in ("two", "one", "frame", "host", "host sampling")}
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(np.zeros(3 * n, F32), np.tile(np.array([0, 0, 0, 1], F32), n), np.ones(3 * n, F32))
        ctx.propagate()
        ctx.anim_upload_tracks(tracks, times, values)
        ctx.anim_upload_targets(single)
        ctx.anim_upload_blend_targets(targets, bindings)

        def timed(key, fn, keep):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.propagate(0)
            ctx.synchronize()
            if keep:
                took[key].append(time.perf_counter() - t0)

        def host_path(x, keep):
            t0 = time.perf_counter()
            a, b = host_sample(clips[0][1], vals[0], x[0::2]), host_sample(clips[1][1], vals[1], x[1::2])
            t, r, s = [p + (q - p) * F32(0.7) for p, q in zip(a, b)]  # (u = 0.7 / (0.3 + 0.7); rotations: the cheaper nlerp, no sign flip)
            r /= np.linalg.norm(r, axis=1, keepdims=True)
            if keep:
                took["host sampling"].append(time.perf_counter() - t0)
            ctx.upload_transforms_indexed(rows, t.reshape(-1), r.reshape(-1), s.reshape(-1))

        for rep in range(reps + 5):  # (five warm-up frames; the four paths alternate)
            two["seek_time"] = rng.uniform(0.01, 0.99, 2 * rigs)
            one["seek_time"] = two["seek_time"][0::2]
            timed("two", lambda: ctx.anim_frame_blended(rigs, two), rep >= 5)
            timed("one", lambda: ctx.anim_frame_blended(rigs, one), rep >= 5)
            timed("frame", lambda: ctx.anim_frame(one["seek_time"]), rep >= 5)
            timed("host", lambda: host_path(two["seek_time"], rep >= 5), rep >= 5)
    print(f"{rigs} rigs x {JOINTS} joints, {reps} frames, wall clock around synchronize:")
    print(f"  anim_frame_blended, two layers (0.3 / 0.7) + propagate             {quartiles(took['two'])}")
    print(f"  anim_frame_blended, one layer + propagate                          {quartiles(took['one'])}")
    print(f"  anim_frame (the same tracks and seek times) + propagate            {quartiles(took['frame'])}")
    print(f"  numpy sampling and blending + upload_transforms_indexed + propagate {quartiles(took['host'])}  (sampling and blending alone {quartiles(took['host sampling'])})")


def graph_deviation():
    import test_gpu_anim_graph as T
    cases = [(f"{name}, {lay}", T.nested_scene(name, lay)) for name, lay in T.NESTED] + [(what, T.mask_scene(what)) for what in T.MASKS]
    rot, lerp = {name: 0.0 for name in T.SHAPES}, 0.0
    for what, sc in cases:
        sc["rot_bound"] = [-1.0 - g for g in range(len(sc["names"]))]  # (a marker per graph in place of the bound)
        (w64, bound), (w32, _) = [T.expected(sc, dt) for dt in (np.float64, F32)]  # (both runs assert the slerps' preconditions)
        for c in range(3):
            exact, err = bound[c] == 0, np.abs(w32[c] - w64[c])
            assert np.array_equal(w32[c][exact], w64[c][exact]), (what, c)
            for g, name in enumerate(sc["names"]):
                rot[name] = max(rot[name], np.max(err[bound[c] == -1.0 - g], initial=0.0) / T.E)
            rest = bound[c] > 0
            lerp = max(lerp, np.max(err[rest] / bound[c][rest], initial=0.0))
    print(f"float32 numpy against float64 over the {len(cases)} nested and mask cases (T.SEEDS): translation / scale and single clips worst error / bound {lerp:.2f}")
    for name, dev in rot.items():
        print(f"  folded rotations of {name}: worst {dev:.2f} x 2^-24 (the test's ROT_DEVIATION: {T.ROT_DEVIATION[name]})")


DEEP = [(2, 0xFFFFFFFF, 0), (1, 0, 0), (1, 1, 0), (0, 2, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]  # add(blend(blend(c0,c1),c2),c3): kind, parent, clip
FLAT = [(1, 0xFFFFFFFF, 0), (0, 0, 0), (0, 0, 1)]                                               # blend(c0,c1)


def graph_ab(rigs, reps):
    """Four clips over the same 24 joints, bindings shared by every rig.  (a) DEEP through anim_frame_graph against its numpy evaluation
    (lerp + normalize for every rotation step, the cheaper arithmetic) + upload_transforms_indexed; (b) FLAT against anim_frame_blended."""
    rng = np.random.default_rng(rigs)
    clips = [clip(rng) for _ in range(4)]
    tracks = np.concatenate([c[0] for c in clips])
    for c in range(1, 4):
        tracks["first_time"][3 * JOINTS * c:3 * JOINTS * (c + 1)] += KEYS * c
        tracks["first_value"][3 * JOINTS * c:3 * JOINTS * (c + 1)] += c * len(clips[0][2])
    times, values = np.concatenate([c[1] for c in clips]), np.concatenate([c[2] for c in clips])
    n = rigs * JOINTS
    bindings = np.zeros(4 * JOINTS, B.ANIM_BINDING_DTYPE)
    for k, f in enumerate(("track_t", "track_r", "track_s")):
        bindings[f] = 3 * JOINTS * (np.arange(4 * JOINTS) % 4) + 3 * (np.arange(4 * JOINTS) // 4) + k
    targets, blend_targets = np.zeros(n, B.ANIM_GRAPH_TARGET_DTYPE), np.zeros(n, B.ANIM_BLEND_TARGET_DTYPE)
    for tg in (targets, blend_targets):
        tg["row"], tg["player"], tg["first_binding"], tg["n_clips"] = np.arange(n), np.arange(n) // JOINTS, 4 * (np.arange(n) % JOINTS), 4
    vals = [[np.stack([c[2][c[0][3 * j + k]["first_value"]:][:KEYS * w].reshape(KEYS, w) for j in range(JOINTS)]) for k, w in enumerate((3, 4, 3))] for c in clips]
    nodes = np.array([(*nd, 0, 0) for nd in DEEP + FLAT], B.ANIM_GRAPH_NODE_DTYPE)
    graphs = np.array([(0, len(DEEP)), (len(DEEP), len(FLAT))], B.ANIM_GRAPH_DTYPE)
    w_deep, w_flat = np.array([1, 0.8, 0.6, 0.3, 0.7, 0.5, 0.25], F32), np.array([1, 0.3, 0.7], F32)
    deep, flat, layers = np.zeros(7 * rigs, B.ANIM_NODE_STATE_DTYPE), np.zeros(3 * rigs, B.ANIM_NODE_STATE_DTYPE), np.zeros(2 * rigs, B.ANIM_LAYER_DTYPE)
    deep["weight"], flat["weight"] = np.tile(w_deep, rigs), np.tile(w_flat, rigs)
    layers["player"], layers["clip"], layers["weight"] = np.arange(2 * rigs) // 2, np.arange(2 * rigs) % 2, np.tile(w_flat[1:], rigs)
    rows = np.arange(n, dtype=U32)
    took = {k: [] for k in ("deep", "host", "host evaluation", "flat", "blended")}
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(np.zeros(3 * n, F32), np.tile(np.array([0, 0, 0, 1], F32), n), np.ones(3 * n, F32))
        ctx.propagate()
        ctx.anim_upload_tracks(tracks, times, values)
        ctx.anim_upload_blend_targets(blend_targets, bindings)
        ctx.anim_upload_graphs(graphs, nodes)

        def timed(key, fn, keep):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.propagate(0)
            ctx.synchronize()
            if keep:
                took[key].append(time.perf_counter() - t0)

        def host_path(x, keep):
            t0 = time.perf_counter()
            v = [host_sample(clips[c][1], vals[c], x[:, c]) for c in range(4)]
            unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)
            out = []
            for k in range(3):
                inner = v[0][k] + (v[1][k] - v[0][k]) * F32(0.7)  # u = 0.7 / (0.3 + 0.7)
                outer = inner + (v[2][k] - inner) * F32(0.5 / 1.1)
                if k != 1:
                    out.append(outer + v[3][k] * F32(0.25))
                    continue
                a, b = unit(np.array([0, 0, 0, 1], F32) + (v[3][k] - np.array([0, 0, 0, 1], F32)) * F32(0.25)).T, unit(unit(inner) + (v[2][k] - unit(inner)) * F32(0.5 / 1.1)).T
                out.append(np.stack([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], axis=1))
            if keep:
                took["host evaluation"].append(time.perf_counter() - t0)
            ctx.upload_transforms_indexed(rows, *[np.ascontiguousarray(o, F32).reshape(-1) for o in out])

        for which, first, run in ((0, 7 * np.arange(rigs), ("deep", "host")), (1, 3 * np.arange(rigs), ("flat", "blended"))):
            ctx.anim_upload_graph_targets(targets, bindings, np.full(rigs, which, U32))
            for rep in range(reps + 5):  # (five warm-up frames; the two paths alternate)
                x = rng.uniform(0.01, 0.99, (rigs, 4)).astype(F32)
                deep["seek_time"].reshape(rigs, 7)[:, [3, 4, 5, 6]] = x
                flat["seek_time"].reshape(rigs, 3)[:, 1:] = x[:, :2]
                layers["seek_time"] = x[:, :2].reshape(-1)
                if which == 0:
                    timed("deep", lambda: ctx.anim_frame_graph(first, deep), rep >= 5)
                    timed("host", lambda: host_path(x, rep >= 5), rep >= 5)
                else:
                    timed("flat", lambda: ctx.anim_frame_graph(first, flat), rep >= 5)
                    timed("blended", lambda: ctx.anim_frame_blended(rigs, layers), rep >= 5)
    print(f"{rigs} rigs x {JOINTS} joints, {reps} frames, wall clock around synchronize:")
    print(f"  (a) anim_frame_graph, add(blend(blend(c0,c1),c2),c3) + propagate        {quartiles(took['deep'])}")
    print(f"      numpy evaluation + upload_transforms_indexed + propagate             {quartiles(took['host'])}  (the evaluation alone {quartiles(took['host evaluation'])})")
    print(f"  (b) anim_frame_graph, blend(c0,c1) at 0.3 / 0.7 + propagate              {quartiles(took['flat'])}")
    print(f"      anim_frame_blended, the same two layers + propagate                  {quartiles(took['blended'])}")


MORPHS = 52


def weights_ab(rigs, reps):
    """Four clips of one 52-weight linear track each over KEYS times, bindings shared by every rig; the twin scene for anim_frame_graph
    cuts the same keys into 18 translation tracks per clip (the last padded).  No propagate on either side: weights need none."""
    import ctypes as C
    rng = np.random.default_rng(rigs)
    rows = (MORPHS + 2) // 3
    times = np.tile(np.linspace(0, 1, KEYS).astype(F32), 4)
    keys = rng.normal(0, 1, (4, KEYS, 3 * rows)).astype(F32)  # [clip][key][scalar]; the weights are the first 52 scalars of a key
    w_tracks = np.array([(KEYS * c, KEYS, c * KEYS * MORPHS, B.ANIM_LINEAR, MORPHS) for c in range(4)], B.ANIM_WEIGHT_TRACK_DTYPE)
    w_values = np.concatenate([keys[c, :, :MORPHS].reshape(-1) for c in range(4)])
    t_tracks = np.array([(KEYS * c, KEYS, (c * rows + j) * KEYS * 3, B.ANIM_TRANSLATION | B.ANIM_LINEAR) for c in range(4) for j in range(rows)], B.ANIM_TRACK_DTYPE)
    t_values = np.concatenate([keys[c, :, 3 * j:3 * j + 3].reshape(-1) for c in range(4) for j in range(rows)])
    morph = np.zeros(rigs, B.ANIM_MORPH_TARGET_DTYPE)
    morph["player"], morph["first_weight"], morph["n_weights"], morph["n_clips"] = np.arange(rigs), MORPHS * np.arange(rigs), MORPHS, 4
    n = rigs * rows
    targets, bindings = np.zeros(n, B.ANIM_GRAPH_TARGET_DTYPE), np.full(4 * rows, B.ANIM_NO_TRACK, B.ANIM_BINDING_DTYPE)
    targets["row"], targets["player"], targets["first_binding"], targets["n_clips"] = np.arange(n), np.arange(n) // rows, 4 * (np.arange(n) % rows), 4
    bindings["track_t"] = rows * (np.arange(4 * rows) % 4) + np.arange(4 * rows) // 4
    nodes = np.array([(*nd, 0, 0) for nd in DEEP + [(0, 0xFFFFFFFF, 0)]], B.ANIM_GRAPH_NODE_DTYPE)
    graphs = np.array([(0, len(DEEP)), (len(DEEP), 1)], B.ANIM_GRAPH_DTYPE)
    deep, single = np.zeros(7 * rigs, B.ANIM_NODE_STATE_DTYPE), np.zeros(rigs, B.ANIM_NODE_STATE_DTYPE)
    deep["weight"], single["weight"] = np.tile(np.array([1, 0.8, 0.6, 0.3, 0.7, 0.5, 0.25], F32), rigs), 1
    hip = C.CDLL("libamdhip64.so")
    took = {}
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(np.zeros(3 * n, F32), np.tile(np.array([0, 0, 0, 1], F32), n), np.ones(3 * n, F32))
        ctx.propagate()
        ctx.anim_upload_tracks(t_tracks, times, t_values)
        ctx.anim_upload_weight_tracks(w_tracks, times, w_values)
        ctx.anim_upload_graphs(graphs, nodes)

        def timed(key, fn, keep):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if keep:
                took.setdefault(key, []).append(time.perf_counter() - t0)

        def host_path(x, which, out_ptr):
            t = times[:KEYS]
            i = np.clip(np.searchsorted(t, x, side="right") - 1, 0, KEYS - 2)  # [rigs, 4]
            u = ((x - t[i]) / (t[i + 1] - t[i])).astype(F32)[:, :, None]
            v = [keys[c, i[:, c], :MORPHS] + (keys[c, i[:, c] + 1, :MORPHS] - keys[c, i[:, c], :MORPHS]) * u[:, c] for c in range(4 if which == 0 else 1)]
            if which == 0:
                inner = v[0] + (v[1] - v[0]) * F32(0.7)
                v[0] = (inner + (v[2] - inner) * F32(0.5 / 1.1)) + v[3] * F32(0.25)
            out = np.ascontiguousarray(v[0], F32)
            assert hip.hipMemcpy(C.c_void_p(out_ptr), C.c_void_p(out.ctypes.data), C.c_size_t(out.nbytes), 1) == 0

        for which, first, states, name in ((0, 7 * np.arange(rigs), deep, "seven nodes"), (1, np.arange(rigs), single, "root CLIP")):
            ctx.anim_upload_morph_targets(morph, np.arange(4), np.full(rigs, which, U32), MORPHS * rigs)
            ctx.anim_upload_graph_targets(targets, bindings, np.full(rigs, which, U32))
            out_ptr = ctx.device_buffer(B.BUF_MORPH_WEIGHTS)[0]
            for rep in range(reps + 5):  # (five warm-up frames; the three paths alternate)
                x = rng.uniform(0.01, 0.99, (rigs, 4)).astype(F32)
                if which == 0:
                    deep["seek_time"].reshape(rigs, 7)[:, [3, 4, 5, 6]] = x
                else:
                    single["seek_time"] = x[:, 0]
                timed(name + ": anim_frame_weights", lambda: ctx.anim_frame_weights(first, states), rep >= 5)
                timed(name + ": numpy evaluation + one hipMemcpy", lambda: host_path(x, which, out_ptr), rep >= 5)
                timed(name + f": anim_frame_graph, {rows} translation targets a rig", lambda: ctx.anim_frame_graph(first, states), rep >= 5)
    print(f"{rigs} rigs x {MORPHS} morph weights, {reps} frames, wall clock around synchronize:")
    for key, xs in took.items():
        print(f"  {key:75s} {quartiles(xs)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--deviation", action="store_true")
    ap.add_argument("--rigs", default="1000,40000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blend", action="store_true")
    ap.add_argument("--blend-deviation", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--graph-deviation", action="store_true")
    ap.add_argument("--weights", action="store_true")
    a = ap.parse_args()
    if a.deviation:
        deviation()
    elif a.graph_deviation:
        graph_deviation()
    elif a.weights:
        for rigs in a.rigs.split(","):
            weights_ab(int(rigs), a.reps)
    elif a.graph:
        for rigs in a.rigs.split(","):
            graph_ab(int(rigs), a.reps)
    elif a.blend_deviation:
        blend_deviation()
    elif a.blend:
        for rigs in a.rigs.split(","):
            blend_ab(int(rigs), a.reps)
    else:
        for rigs in a.rigs.split(","):
            ab(int(rigs), a.reps)
