"""mi_anim_frame (keyframe tracks sampled into Transforms on the device) against `sample` below: a plain numpy restatement of the
sampling include/bevy_mi355x.h states, evaluated in float64 on the float32 inputs (branch decisions included).  Bounds, with
e = 2^-24 (tools/probes/animation_probe.py re-measures a float32 run of `sample` on these very inputs: profiles/r10_animation/ab.md):
  step, clamped ends, exact key hits   bit for bit
  linear translation / scale           8 e (|a| + |b|): three roundings of u, three of the lerp (the issue's bound)
  cubic translation / scale            24 e S, S = |a| + |b| + d (|out| + |in|).  u carries 3 e; through the basis functions' slopes (at
      most 1.5, and 1 x d) that is 4.5 e on h00 / h01 and 3 e d on h10 / h11.  Their own arithmetic from u2 (1 rounding) and u3 (2):
      h00 <= 12 e, h01 <= 11 e, h10 <= 7 e d, h11 <= 5 e d.  Each product adds 1 e of its term, each of the three sums 1 e S.
      Worst term: (4.5 + 12 + 1) e |a|, plus 3 e S: 20.5 e S, rounded up to 24.
  rotations (slerp; cubic + normalize) 16 e absolute per component: four times the 4.1 e a float32 numpy run deviates (the device's
      acos / sin are not numpy's).  Re-measured on these inputs: 4.11 e, for which the rule would allow 16.4 e; the test keeps 16.
Measured on an MI355X: the worst error of any case is 0.26 of its bound."""
import ctypes as C

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api, workloads as W

pytestmark = pytest.mark.gpu

F32, F64, U32 = np.float32, np.float64, np.uint32
E = 2.0 ** -24
STEP, LINEAR, CUBIC = B.ANIM_STEP, B.ANIM_LINEAR, B.ANIM_CUBIC
COMPS = (B.ANIM_TRANSLATION, B.ANIM_ROTATION, B.ANIM_SCALE)
SEEKS = (0.1, 0.25, 0.5, 0.6180339, 0.75, 0.9)  # below T[0], T[0], an interior key (k >= 3), inside an interval, T[k-1], above


def sample(T, V, rot, interp, x, dt=F64):
    """One track at x in dtype dt -> (value, bound; 0 = bit for bit).  V: [k, w], or [k, 3, w] (in, value, out) for CUBIC."""
    T, V, x, k = T.astype(dt), V.astype(dt), dt(x), len(T)
    val = (lambda i: V[i, 1]) if interp == CUBIC else (lambda i: V[i])
    if k == 1 or not x > T[0]:
        return val(0), 0.0
    if x >= T[-1]:
        return val(k - 1), 0.0
    i = int(np.searchsorted(T, x, side="right")) - 1
    if interp == STEP or x == T[i]:
        return val(i), 0.0
    d = T[i + 1] - T[i]
    u = (x - T[i]) / d
    a, b = val(i), val(i + 1)
    norm = lambda q: q / np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    if interp == LINEAR and not rot:
        return a + (b - a) * u, 8 * E * (abs(a) + abs(b))
    if interp == LINEAR:
        dot = (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3])
        if dot < 0:
            b, dot = -b, -dot
        if dot > dt(0.9995):
            return norm(a + (b - a) * u), 16 * E
        th = np.arccos(dot)
        return (a * np.sin(th * (1 - u)) + b * np.sin(th * u)) * (1 / np.sin(th)), 16 * E
    to, ti = V[i, 2], V[i + 1, 0]
    u2 = u * u
    u3 = u2 * u
    h00, h10, h01, h11 = (2 * u3 - 3 * u2) + 1, d * ((u3 - 2 * u2) + u), 3 * u2 - 2 * u3, d * (u3 - u2)
    q = ((h00 * a + h10 * to) + h01 * b) + h11 * ti
    return (norm(q), 16 * E) if rot else (q, 24 * E * (abs(a) + abs(b) + d * (abs(to) + abs(ti))))


def key_times(rng, k):
    """k ascending times from 0.25 to 0.75 with 0.5 among them (k >= 3): SEEKS hits every case on every track"""
    fixed = [0.25, 0.75, 0.5][:k]
    return np.sort(np.array(fixed + list(rng.uniform(0.26, 0.74, k - len(fixed))), F32))


def quat_keys(rng, k, phase):
    """Unit quaternions whose consecutive pairs cycle through: dot in (0.05, 0.95), dot in (-0.95, -0.05), dot > 0.9995 (1e-2 apart),
    identical -- built, so that |dot| > 1e-3 and |dot - 0.9995| > 1e-4 hold for every pair"""
    q = [rng.normal(size=4)]
    q[0] /= np.linalg.norm(q[0])
    for j in range(1, k):
        p, o = q[-1], rng.normal(size=4)
        o -= p * (o @ p)
        o /= np.linalg.norm(o)
        c = rng.uniform(0.05, 0.95)
        kind = (j + phase) % 4
        q.append([c * p + np.sqrt(1 - c * c) * o, -c * p + np.sqrt(1 - c * c) * o, (p + 1e-2 * o) / np.sqrt(1 + 1e-4), p][kind])
    return np.array(q, F32)


def build(rng, n_targets, n_rows, interp, k, layout):
    """-> tracks, times, values, targets, per target [(T, V) or None] x 3.  layout: shared = every track reads one range of times;
    own = each its own, of k + (0, 1, 2) keys; mixed = own in the first 32 targets (half a wave), shared behind.  Target i tracks the
    components (i % 7) + 1 (one, two and all three occur); players 0 / 1 alternate, so both meet inside a wave after the sort."""
    times, values, tracks, per, n_t, n_v = [], [], [], [], 0, 0
    shared = key_times(rng, k)
    times.append(shared)
    n_t = k
    rows = rng.permutation(n_rows)[:n_targets].astype(U32)
    targets = np.zeros(n_targets, B.ANIM_TARGET_DTYPE)
    for i in range(n_targets):
        idx, tv = [B.ANIM_NO_TRACK] * 3, [None] * 3
        for c in range(3):
            if not ((i % 7) + 1) >> c & 1:
                continue
            own = layout == "own" or (layout == "mixed" and i < 32)
            kk = k + (i + c) % 3 if own else k
            T, first = (key_times(rng, kk), n_t) if own else (shared, 0)
            if own:
                times.append(T)
                n_t += kk
            w = 4 if c == 1 else 3
            V = quat_keys(rng, kk, i + c) if c == 1 else rng.normal(0, 2, (kk, w)).astype(F32)
            if interp == CUBIC:
                V = np.stack([rng.normal(0, 0.3, (kk, w)).astype(F32), V, rng.normal(0, 0.3, (kk, w)).astype(F32)], axis=1)
            idx[c], tv[c] = len(tracks), (T, V)
            tracks.append((first, kk, n_v, COMPS[c] | interp))
            values.append(V.reshape(-1))
            n_v += V.size
        targets[i] = (rows[i], i % 2, *idx)
        per.append(tv)
    return np.array(tracks, B.ANIM_TRACK_DTYPE), np.concatenate(times), np.concatenate(values), targets, per


def read_columns(ctx):
    hip, out = C.CDLL("libamdhip64.so"), []
    ctx.synchronize()
    for which, w in ((api.BUF_TRANSLATION, 3), (api.BUF_ROTATION, 4), (api.BUF_SCALE, 3)):
        a = np.zeros((ctx.n, w), F32)
        p, nbytes = ctx.device_buffer(which)
        assert nbytes == a.nbytes and hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(p), C.c_size_t(nbytes), 2) == 0
        out.append(a)
    return out


CASES = [(65, i, k, lay) for i in (STEP, LINEAR, CUBIC) for k in (1, 2, 3, 70) for lay in ("shared", "own", "mixed")]
CASES += [(n, LINEAR, 3, "shared") for n in (1, 63, 64, 257)] + [(257, CUBIC, 70, "own")]


@pytest.mark.parametrize("n_targets,interp,k,layout", CASES)
def test_sampling(n_targets, interp, k, layout):
    rng = np.random.default_rng(1000 * n_targets + 100 * interp + k)
    n = n_targets + 40
    tracks, times, values, targets, per = build(rng, n_targets, n, interp, k, layout)
    cur = [rng.normal(0, 1, (n, w)).astype(F32) for w in (3, 4, 3)]
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(*[c.reshape(-1) for c in cur])
        ctx.propagate()  # (consumes the rows' Added<GlobalTransform>: the change bytes below are the frame's alone)
        ctx.anim_upload_tracks(tracks, times, values)
        ctx.anim_upload_targets(targets)
        for j in range(len(SEEKS)):
            seeks = np.array([SEEKS[j], SEEKS[(j + 3) % 6]], F32)
            ctx.anim_frame(seeks)
            want, bound = [c.astype(F64) for c in cur], [np.zeros((n, w)) for w in (3, 4, 3)]
            for tg, tv in zip(targets, per):
                for c in range(3):
                    if tv[c] is not None:
                        want[c][tg["row"]], bound[c][tg["row"]] = sample(*tv[c], c == 1, interp, seeks[tg["player"]])
            cur = read_columns(ctx)
            for c, got in enumerate(cur):
                exact = bound[c] == 0  # untracked components and rows no target writes among them
                assert np.array_equal(got.view(U32)[exact], want[c].astype(F32).view(U32)[exact]), (j, c)
                err = np.abs(got - want[c])
                print(f"seek {j} component {c}: max error / bound {np.max(err[~exact] / bound[c][~exact], initial=0.0):.3f}")
                assert np.all(err[~exact] <= bound[c][~exact]), (j, c)
            if j == 0:
                ctx.propagate(0)
                assert np.array_equal(ctx.download_changed_global_transforms()[0], np.sort(targets["row"]))


@pytest.mark.parametrize("hierarchy", [True, False])
def test_state_equals_an_indexed_upload(hierarchy):
    """anim_frame + the frame call against an indexed upload of the reference-sampled Transforms + the frame call on a twin context:
    GlobalTransforms, change ticks, changed-row list and masks after each of two frames (step tracks: the samples are exact)."""
    rng = np.random.default_rng(7)
    n = 300
    parent = np.full(n, B.NO_PARENT, U32)  # level 0: rows [0, 130), ten of them with children; level 1: [130, 180); level 2: [180, 300)
    parent[130:180], parent[180:] = np.arange(50) // 5, 130 + np.arange(120) * 5 // 12
    tracks, times, values, targets, per = build(rng, 130, n, STEP, 3, "mixed")
    cols = [rng.normal(0, 3, (n, 3)).astype(F32), quat_keys(rng, n, 0), np.ones((n, 3), F32)]
    cfv = api.perspective_clip_from_view(W.CAMERA_FOV, W.CAMERA_ASPECT, W.CAMERA_NEAR)
    frusta = api.compute_frustum(cfv, W.many_cubes_camera(0, position=(0.0, 0.0, 30.0)), W.CAMERA_FAR)
    flags = B.CULL_BEGIN_FRAME | B.CULL_END_FRAME | (B.CULL_STATIC_OPT if hierarchy else 0)
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            ctx.resize(n)
            ctx.upload_transforms(*[c.reshape(-1) for c in cols])
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            if hierarchy:
                ctx.upload_hierarchy(parent, [0, 130, 180, n])
            ctx.propagate_and_cull(frusta, flags=flags)
        a.anim_upload_tracks(tracks, times, values)
        a.anim_upload_targets(targets)
        for seeks in ([0.3, 0.6], [0.3, 0.8]):  # (player 0 stays where it was in the second frame)
            a.anim_frame(seeks)
            for tg, tv in zip(targets, per):
                for c in range(3):
                    if tv[c] is not None:
                        cols[c][tg["row"]] = sample(*tv[c], c == 1, STEP, F32(seeks[tg["player"]]))[0]
            rows = targets["row"]
            b.upload_transforms_indexed(rows, *[c[rows].reshape(-1) for c in cols])
            for ctx in (a, b):
                ctx.propagate_and_cull(frusta, flags=flags | B.CULL_CHANGED_ROWS)
            (ga, ca), (gb, cb) = a.download_global_transforms(), b.download_global_transforms()
            assert ga.tobytes() == gb.tobytes() and np.array_equal(ca, cb)
            assert np.array_equal(a.download_changed_global_transforms()[0], b.download_changed_global_transforms()[0])
            assert np.array_equal(a.download_visibility(0), b.download_visibility(0))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(a), cols))


def altered(p, key, field, at, value):
    q = p[key].copy()
    q[field][at] = value
    return q


BAD = {  # name -> (the refused call, its error)
    "descending times": (lambda ctx, p: ctx.anim_upload_tracks(p["tracks"], p["times"][::-1], p["values"]), api.MI_ERR_INVALID_ARG),
    "range past its pool": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "first_value", -1, p["tracks"]["first_value"][-1] + 1), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "rotation track in a translation field": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "track_t", 0, p["targets"]["track_r"][1])), api.MI_ERR_INVALID_ARG),
    "duplicate rows": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "row", 1, p["targets"]["row"][0])), api.MI_ERR_INVALID_ARG),
    "row >= n": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "row", 0, ctx.n)), api.MI_ERR_INVALID_ARG),
    "frame before the uploads": (None, api.MI_ERR_NOT_READY),
    "n_players too small": (lambda ctx, p: ctx.anim_frame([0.5]), api.MI_ERR_INVALID_ARG),
    "frame after a shrinking resize": (lambda ctx, p: (ctx.resize(int(p["targets"]["row"].max())), ctx.anim_frame([0.5, 0.5])), api.MI_ERR_NOT_READY),
}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_checks(what):
    rng = np.random.default_rng(3)
    n = 20
    tracks, times, values, targets, per = build(rng, 8, n, LINEAR, 3, "shared")  # (target 0 tracks its translation alone, target 1 its rotation)
    p = dict(tracks=tracks, times=times, values=values, targets=targets)
    call, code = BAD[what]
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(np.zeros(3 * n, F32), np.tile(np.array([0, 0, 0, 1], F32), n), np.ones(3 * n, F32))
        with pytest.raises(B.MiError) as e:
            if call is None:
                ctx.anim_frame([0.5, 0.5])
            ctx.anim_upload_tracks(tracks, times, values)
            ctx.anim_upload_targets(targets)
            call(ctx, p)
        assert e.value.code == code
        ctx.resize(n)  # the state from before the refused call serves a frame (the uploads are made now where the frame came first)
        if call is None:
            ctx.anim_upload_tracks(tracks, times, values)
            ctx.anim_upload_targets(targets)
        ctx.anim_frame([0.5, 0.5])
        want = sample(times[:3], values[:9].reshape(3, 3), False, LINEAR, 0.5)[0].astype(F32)  # (0.5 is a key: bit for bit)
        assert np.array_equal(read_columns(ctx)[0][targets["row"][0]], want)
