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
Measured on an MI355X: the worst error of any case is 0.26 of its bound.
Behind those 51 cases, 57 more (NEW_CASES and the tests after it): anim_wave_interval's rounds at their seams with index-encoded tracks,
staged next to unstaged workgroups, NaN / inf / -0.0 seek times, 200 sparse players with trackless targets, the state seams against
an indexed upload on a twin context, and two rigs through anim_frame -> propagate -> skin_frame.  The same comparisons and bounds;
the worst error of the bounded ones among them is 0.23 of its bound (a float32 run of the reference: 0.22)."""
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


def build(rng, n_targets, n_rows, interp, k, layout, players=None, trackless=(), rows=None, shuffle=False):
    """-> tracks, times, values, targets, per target [(T, V) or None] x 3.  layout: shared = every track reads one range of times;
    own = each its own, of k + (0, 1, 2) keys; mixed = own in the first 32 targets (half a wave), shared behind.  Target i tracks the
    components (i % 7) + 1 (one, two and all three occur); players 0 / 1 alternate, so both meet inside a wave after the sort.
    players: target i's player instead; trackless: the targets with no track at all; rows: the targets' rows instead of random ones;
    shuffle: the targets are handed over in a random order."""
    times, values, tracks, per, n_t, n_v = [], [], [], [], 0, 0
    shared = key_times(rng, k)
    times.append(shared)
    n_t = k
    rows = rng.permutation(n_rows)[:n_targets].astype(U32) if rows is None else np.asarray(rows, U32)
    targets = np.zeros(n_targets, B.ANIM_TARGET_DTYPE)
    for i in range(n_targets):
        idx, tv = [B.ANIM_NO_TRACK] * 3, [None] * 3
        for c in range(3):
            if i in trackless or not ((i % 7) + 1) >> c & 1:
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
        targets[i] = (rows[i], i % 2 if players is None else players[i], *idx)
        per.append(tv)
    if shuffle:
        order = rng.permutation(n_targets)
        targets, per = targets[order], [per[j] for j in order]
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


def with_time(p, at, value):
    t = p["times"].copy()
    t[at] = value
    return t


BAD = {  # name -> (the refused call, its error)
    "descending times": (lambda ctx, p: ctx.anim_upload_tracks(p["tracks"], p["times"][::-1], p["values"]), api.MI_ERR_INVALID_ARG),
    "range past its pool": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "first_value", -1, p["tracks"]["first_value"][-1] + 1), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "rotation track in a translation field": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "track_t", 0, p["targets"]["track_r"][1])), api.MI_ERR_INVALID_ARG),
    "duplicate rows": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "row", 1, p["targets"]["row"][0])), api.MI_ERR_INVALID_ARG),
    "row >= n": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "row", 0, ctx.n)), api.MI_ERR_INVALID_ARG),
    "frame before the uploads": (None, api.MI_ERR_NOT_READY),
    "n_players too small": (lambda ctx, p: ctx.anim_frame([0.5]), api.MI_ERR_INVALID_ARG),
    "no keys": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "n_keys", 0, 0), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "unknown interpolation": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "kind_interp", 0, COMPS[0] | 3), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "unknown component": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "kind_interp", 0, 0x30 | LINEAR), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "times past their pool": (lambda ctx, p: ctx.anim_upload_tracks(altered(p, "tracks", "first_time", -1, len(p["times"]) - 2), p["times"], p["values"]), api.MI_ERR_INVALID_ARG),
    "equal adjacent times": (lambda ctx, p: ctx.anim_upload_tracks(p["tracks"], with_time(p, 1, p["times"][0]), p["values"]), api.MI_ERR_INVALID_ARG),
    "a NaN time": (lambda ctx, p: ctx.anim_upload_tracks(p["tracks"], with_time(p, 1, np.nan), p["values"]), api.MI_ERR_INVALID_ARG),
    "track index >= pool size": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "track_t", 0, len(p["tracks"]))), api.MI_ERR_INVALID_ARG),
    "player 0xFFFFFFFF": (lambda ctx, p: ctx.anim_upload_targets(altered(p, "targets", "player", 0, 0xFFFFFFFF)), api.MI_ERR_INVALID_ARG),
    "frame flags": (lambda ctx, p: ctx._ck(ctx._lib.mi_anim_frame(ctx._h, 2, api._ptr(np.full(2, 0.5, F32), C.c_float), C.c_uint32(1))), api.MI_ERR_INVALID_ARG),
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


# ---- the search seams, seek-time edges, many players: cases built without a device, so that tools/probes/animation_probe.py can run
# ---- the float32 reference over the very same inputs (NEW_CASES below)
NO = B.ANIM_NO_TRACK


def expected(cur, targets, per, seeks, interp=None, dt=F64):
    """The columns an anim_frame at `seeks` leaves behind over `cur` -> want [3] in dt, bound [3] (0 = bit for bit).
    per[i][c] = (T, V) or (T, V, interp) or None; targets that share a track and a seek time are sampled once."""
    want, bound, memo = [c.astype(dt) for c in cur], [np.zeros(c.shape) for c in cur], {}
    for tg, tv in zip(targets, per):
        for c in range(3):
            if tv[c] is None:
                continue
            T, V, ip = (*tv[c], interp)[:3]
            x = seeks[tg["player"]]
            key = (id(T), id(V), ip, x.tobytes())
            if key not in memo:
                memo[key] = sample(T, V, c == 1, ip, x, dt)
            want[c][tg["row"]], bound[c][tg["row"]] = memo[key]
    return want, bound


def compare(got, want, bound, what):
    """bit for bit where the bound is 0, inside it elsewhere -> the worst error / bound"""
    worst = 0.0
    for c in range(3):
        exact = bound[c] == 0
        assert np.array_equal(got[c].view(U32)[exact], want[c].astype(F32).view(U32)[exact]), (what, c)
        err = np.abs(got[c] - want[c])
        worst = max(worst, np.max(err[~exact] / bound[c][~exact], initial=0.0))
        assert np.all(err[~exact] <= bound[c][~exact]), (what, c)
    print(f"{what}: max error / bound {worst:.3f}")
    return worst


def search_times(k):
    return (F32(0.25) + np.arange(k, dtype=F32) / F32(16384)).astype(F32)  # (exact: multiples of 2^-14 below 1)


def search_positions(k):
    """-> seek times f32[p] around the seams of anim_wave_interval's rounds over k keys, and the interval each has to find: on the
    keys 0, 1, s-1, s, s+1, 63s-1, 63s, k-2, k-1 for the first round's stride s (and, where a second round follows, on the same
    offsets of its stride inside two blocks of the first), at the midpoint behind each, and one ulp either side of keys s and k-2.
    No two neighbours are equal: with 32 targets per player every wave holds two different seek times."""
    T, s = search_times(k), (k + 63) // 64
    keys = {0, 1, s - 1, s, s + 1, 63 * s - 1, 63 * s, k - 2, k - 1}
    if s > 64:  # a block of s keys goes through a second round, stride s2
        s2 = (s + 63) // 64
        keys |= {m * s + o for m in (1, 31) for o in (0, 1, s2 - 1, s2, s2 + 1, s - 2, s - 1)}
    seeks, index = [], []
    for i in sorted(j for j in keys if 0 <= j < k):
        seeks.append(T[i]), index.append(i)
        if i + 1 < k:
            seeks.append((T[i] + T[i + 1]) / F32(2)), index.append(i)  # (exact: a multiple of 2^-15)
    for i in (s, k - 2):
        seeks += [np.nextafter(T[i], F32(-np.inf)), np.nextafter(T[i], F32(np.inf))]
        index += [i - 1, i]
    seeks = np.array(seeks, F32)
    assert np.all(seeks[1:] != seeks[:-1])
    return seeks, np.array(index)


def search_pool(k):
    """Index-encoded tracks over T = search_times(k), key i = (i, i, i[, i]): 0 translation STEP, 1 rotation STEP (un-normalised:
    STEP hands it back bit for bit), 2 translation LINEAR, 3 scale LINEAR; and behind them in both pools 4, a translation LINEAR track
    of 3 keys (what reads past the long track's end stays inside the pools)."""
    T, idx = search_times(k), np.arange(k, dtype=F32)
    V3, V4 = np.repeat(idx, 3).reshape(k, 3), np.repeat(idx, 4).reshape(k, 4)
    short_T, short_V = np.array([0.25, 0.5, 0.75], F32), np.arange(100, 109, dtype=F32).reshape(3, 3)
    tracks = np.array([(0, k, 0, COMPS[0] | STEP), (0, k, 3 * k, COMPS[1] | STEP), (0, k, 0, COMPS[0] | LINEAR), (0, k, 0, COMPS[2] | LINEAR),
                       (k, 3, 7 * k, COMPS[0] | LINEAR)], B.ANIM_TRACK_DTYPE)
    return tracks, np.concatenate([T, short_T]), np.concatenate([V3.reshape(-1), V4.reshape(-1), short_V.reshape(-1)]), (T, V3, V4, short_T, short_V)


def targets_of(rows, players, track_t, track_r, track_s):
    tg = np.zeros(len(rows), B.ANIM_TARGET_DTYPE)
    tg["row"], tg["player"], tg["track_t"], tg["track_r"], tg["track_s"] = rows, players, track_t, track_r, track_s
    return tg


SEARCH_K = (64, 65, 128, 129, 130, 2048, 2049, 4096, 4097)  # 130: stride 3 with a last block of one key


def case_search(mode, k):
    """step / linear: 64 targets per player on consecutive rows, wave p is player p's and searches once (anim_wave_interval);
    lane: 32 per player, every wave holds two seek times and each lane searches for itself (anim_lane_interval), on the same data."""
    tracks, times, values, (T, V3, V4, _, _) = search_pool(k)
    seeks, index = search_positions(k)
    assert np.array_equal(np.searchsorted(T, seeks, side="right") - 1, index)  # the recipe produces the intervals it is meant to
    each = 32 if mode == "lane" else 64
    n = each * len(seeks)
    pick = {"step": (0, 1, NO), "linear": (2, NO, 3), "lane": (2, 1, 3)}[mode]
    tv = [(T, V3, STEP if mode == "step" else LINEAR), (T, V4, STEP), (T, V3, LINEAR)]
    per = [[tv[c] if pick[c] != NO else None for c in range(3)]] * n
    return dict(n=n, tracks=tracks, times=times, values=values, targets=targets_of(np.arange(n), np.arange(n) // each, *pick), per=per,
                seeks=[seeks], index=index, each=each)


def case_staging(which):
    if which == "unstaged and staged workgroups":
        # workgroup 0 (players 0..3) reads the 2049-key range where it lies; workgroup 1 (players 4, 5) stages the 3 keys behind it: lo = 2049
        tracks, times, values, (T, V3, V4, short_T, short_V) = search_pool(2049)
        n = 384
        players = np.arange(n) // 64
        long = players < 4
        targets = targets_of(np.arange(n), players, np.where(long, 2, 4), np.where(long, 1, NO), np.where(long, 3, NO))
        per = [[(T, V3, LINEAR), (T, V4, STEP), (T, V3, LINEAR)] if l else [(short_T, short_V, LINEAR), None, None] for l in long]
        seeks = np.array([(T[1000] + T[1001]) / F32(2), T[2047], np.nextafter(T[2048], F32(0)), (T[0] + T[1]) / F32(2), 0.3, 0.6], F32)
        return dict(n=n, tracks=tracks, times=times, values=values, targets=targets, per=per, seeks=[seeks])
    # one wave, one player, lanes with tracks of 1 and of 4097 keys side by side, each track with times of its own
    T, idx = search_times(4097), np.arange(4097, dtype=F32)
    V, ones = np.repeat(idx, 3).reshape(-1, 3), [(np.array([0.3 + j], F32), np.full((1, 3), 7.0 + j, F32)) for j in range(4)]
    tracks, times, values, tv = [], [], [V.reshape(-1)], []
    for j in range(8):
        if j % 2:
            tracks.append((sum(map(len, times)), 4097, 0, COMPS[0] | LINEAR)), times.append(T), tv.append((T, V, LINEAR))
        else:
            tracks.append((sum(map(len, times)), 1, V.size + 3 * (j // 2), COMPS[0] | LINEAR)), times.append(ones[j // 2][0])
            values.append(ones[j // 2][1].reshape(-1)), tv.append((*ones[j // 2], LINEAR))
    return dict(n=64, tracks=np.array(tracks, B.ANIM_TRACK_DTYPE), times=np.concatenate(times), values=np.concatenate(values),
                targets=targets_of(np.arange(64), 0, np.arange(64) % 8, NO, NO), per=[[tv[i % 8], None, None] for i in range(64)],
                seeks=[np.array([(T[2500] + T[2501]) / F32(2)], F32), np.array([T[4095]], F32)])


EDGE_TIMES = [[0.0], [0.0, 0.5], [-0.5, 0.5], [0.0, 0.125, 0.25, 0.375, 0.5], [-0.5, -0.25, 0.0, 0.25, 0.5]]
EDGE_SEEKS = np.concatenate([np.array([0x7FC00000, 0xFFC00000], U32).view(F32), np.array([np.inf, -np.inf, -0.0, 0.0, -1.0, 2.0], F32)])


def case_seek_edges():
    """Tracks of 1, 2 and 5 keys (first key at +0.0, or negative and positive times), every interpolation, all three components: a group
    of three tracks per (times, interpolation).  Players 4..11 seek NaN, -NaN, +inf, -inf, -0.0, +0.0, below and above all keys, a
    target per group each.  In front of them two whole waves on one group each: wave 0 = players 0 / 1 at -0.0 / +0.0 (equal, other
    bits: not one search), wave 1 = players 2 / 3 at one bit pattern (one search across both), its first five lanes without a
    translation track (the leading lane is lane 5)."""
    rng = np.random.default_rng(11)
    tracks, times, values, groups, n_t, n_v = [], [], [], {}, 0, 0
    for ti, tt in enumerate(EDGE_TIMES):
        T, k = np.array(tt, F32), len(tt)
        times.append(T)
        for interp in (STEP, LINEAR, CUBIC):
            g = []
            for c in range(3):
                V = quat_keys(rng, k, ti + c) if c == 1 else rng.normal(0, 2, (k, 3)).astype(F32)
                if interp == CUBIC:
                    V = np.stack([rng.normal(0, 0.3, V.shape).astype(F32), V, rng.normal(0, 0.3, V.shape).astype(F32)], axis=1)
                g.append((len(tracks), (T, V, interp)))
                tracks.append((n_t, k, n_v, COMPS[c] | interp))
                values.append(V.reshape(-1))
                n_v += V.size
            groups[ti, interp] = g
        n_t += k
    order = list(groups.values())
    use = [groups[4, LINEAR]] * 64 + [groups[4, CUBIC]] * 64 + order * len(EDGE_SEEKS)
    players = np.concatenate([np.arange(128) // 32, 4 + np.arange(len(order) * len(EDGE_SEEKS)) // len(order)])
    idx = np.array([[t[0] for t in g] for g in use], U32)
    per = [[t[1] for t in g] for g in use]
    idx[64:69, 0] = NO
    for i in range(64, 69):
        per[i] = [None, *per[i][1:]]
    n = len(use)
    seeks = np.concatenate([np.array([-0.0, 0.0, 0.1, 0.1], F32), EDGE_SEEKS])
    return dict(n=n, tracks=np.array(tracks, B.ANIM_TRACK_DTYPE), times=np.concatenate(times), values=np.concatenate(values),
                targets=targets_of(np.arange(n), players, *idx.T), per=per, seeks=[seeks])


def case_players(interp, k, layout):
    """200 players of 3 targets (a wave holds 21 of them), numbered 0, 5, 10, ... below an n_players of 1000; every tenth target without
    any track; the targets handed over shuffled."""
    rng = np.random.default_rng(200 + interp)
    tracks, times, values, targets, per = build(rng, 600, 640, interp, k, layout, players=5 * (np.arange(600) // 3), trackless=set(range(9, 600, 10)),
                                                shuffle=True)
    assert sum(all(t is None for t in tv) for tv in per) == 60
    return dict(n=640, tracks=tracks, times=times, values=values, targets=targets, per=[[None if t is None else (*t, interp) for t in tv] for tv in per],
                seeks=[rng.uniform(0.2, 0.8, 1000).astype(F32) for _ in range(2)], changed=True)


NEW_CASES = {f"search {mode} k={k}": (case_search, mode, k) for mode in ("step", "linear", "lane") for k in SEARCH_K}
NEW_CASES.update({f"staging: {w}": (case_staging, w) for w in ("unstaged and staged workgroups", "1 and 4097 keys in one wave")})
NEW_CASES["seek edges"] = (case_seek_edges,)
NEW_CASES.update({f"players {name}": (case_players, *a) for name, a in (("linear shared", (LINEAR, 5, "shared")), ("cubic own", (CUBIC, 3, "own")))})


def run_case(name):
    """The case's frames on a device, every column against `expected` -> the case, the columns after its last frame"""
    fn, *args = NEW_CASES[name]
    case = fn(*args)
    n = case["n"]
    cur = [np.random.default_rng(5).normal(0, 1, (n, w)).astype(F32) for w in (3, 4, 3)]
    with B.Context() as ctx:
        ctx.resize(n)
        ctx.upload_transforms(*[c.reshape(-1) for c in cur])
        ctx.propagate()
        ctx.anim_upload_tracks(case["tracks"], case["times"], case["values"])
        ctx.anim_upload_targets(case["targets"])
        for j, seeks in enumerate(case["seeks"]):
            ctx.anim_frame(seeks)
            want, bound = expected(cur, case["targets"], case["per"], seeks)
            cur = read_columns(ctx)
            compare(cur, want, bound, f"{name}, frame {j}")
            if case.get("changed"):  # every target's row counts as changed; the ones without a track too (their Transform kept its bits above)
                ctx.propagate(0)
                assert np.array_equal(ctx.download_changed_global_transforms()[0], np.sort(case["targets"]["row"]))
    return case, cur, want


@pytest.mark.parametrize("k", SEARCH_K)
@pytest.mark.parametrize("mode", ["step", "linear", "lane"])
def test_interval_search(mode, k):
    """The result names the interval the search found: key i holds i in every component."""
    case, got, want = run_case(f"search {mode} k={k}")
    if mode == "step":  # (no arithmetic at all: the reference's own answer is the index the recipe intends)
        assert np.array_equal(want[0][::case["each"], 0], case["index"]) and np.array_equal(want[1][::case["each"], 3], case["index"])
        assert np.array_equal(got[0][::case["each"], 0], case["index"])


@pytest.mark.parametrize("which", ["unstaged and staged workgroups", "1 and 4097 keys in one wave"])
def test_search_staging(which):
    run_case(f"staging: {which}")


def test_seek_time_edges():
    case, got, _ = run_case("seek edges")
    for c in range(3):  # -0.0 and +0.0 are one seek time
        assert got[c][:32].tobytes() == got[c][32:64].tobytes()
        minus, plus = [got[c][case["targets"]["player"] == p] for p in (8, 9)]
        assert len(minus) == 15 and minus.tobytes() == plus.tobytes()


@pytest.mark.parametrize("name", ["linear shared", "cubic own"])
def test_many_sparse_players_and_trackless_targets(name):
    run_case(f"players {name}")


# ---- state seams: anim_frame against an indexed upload of the reference-sampled rows on a twin context
def view_frustum():
    cfv = api.perspective_clip_from_view(W.CAMERA_FOV, W.CAMERA_ASPECT, W.CAMERA_NEAR)
    return api.compute_frustum(cfv, W.many_cubes_camera(0, position=(0.0, 0.0, 30.0)), W.CAMERA_FAR)


WHOLE = B.CULL_BEGIN_FRAME | B.CULL_END_FRAME


def step_rows(cols, targets, per, seeks):
    """STEP tracks sampled at seeks into cols, in place (exact) -> the targets' rows and their Transforms, as an indexed upload takes them"""
    want, bound = expected(cols, targets, per, np.asarray(seeks, F32), STEP)
    assert not any(b.any() for b in bound)
    for c in range(3):
        cols[c][...] = want[c].astype(F32)
    return rows_of(cols, targets["row"])


def rows_of(cols, rows):
    return (np.asarray(rows, U32), *[c[rows].reshape(-1) for c in cols])


def same_state(a, b, cols, what):
    (ga, ca), (gb, cb) = a.download_global_transforms(), b.download_global_transforms()
    assert ga.tobytes() == gb.tobytes() and np.array_equal(ca, cb), what
    assert np.array_equal(a.download_changed_global_transforms()[0], b.download_changed_global_transforms()[0]), what
    assert np.array_equal(a.download_visibility(0), b.download_visibility(0)), what
    for ctx in (a, b):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(ctx), cols)), what
    return ga.reshape(-1, 12)


@pytest.mark.parametrize("hierarchy", [True, False])
@pytest.mark.parametrize("row", [64, 127, 128, 191])
def test_one_animated_scale_at_the_edge_of_a_uniform_block(row, hierarchy):
    """256 rows of scale ONE, the all-rows frame reads every wave's scale from the row summary; then one target with a scale track, on the
    first or last row of a 64-row block, between targets without one.  mi_anim_frame touches the summary for exactly that row: the
    frame behind it must see the animated scale."""
    n = 256
    rng = np.random.default_rng(row)
    parent = np.full(n, B.NO_PARENT, U32)
    parent[200:] = 3 * np.arange(56) + 1  # level 1: rows [200, 256) under rows 1, 4, ... 166 (64 and 127 among them)
    cols = [rng.integers(-5, 6, (n, 3)).astype(F32), np.tile(np.array([0, 0, 0, 1], F32), (n, 1)), np.ones((n, 3), F32)]
    T = np.array([0.25, 0.75], F32)
    S, Vt = np.array([[2, 0.5, -3], [1, 1, 1]], F32), rng.integers(-5, 6, (5, 2, 3)).astype(F32)
    tracks = np.array([(0, 2, 6 * i, COMPS[0] | STEP) for i in range(5)] + [(0, 2, 30, COMPS[2] | STEP)], B.ANIM_TRACK_DTYPE)
    rows = np.array([3, row - 1, row, row + 1, 250])
    targets = targets_of(rows, 0, np.arange(5), NO, np.where(rows == row, 5, NO))
    per = [[(T, Vt[i]), None, (T, S) if rows[i] == row else None] for i in range(5)]
    frusta = view_frustum()
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            ctx.debug_set_row_summary(0)
            ctx.resize(n)
            ctx.upload_transforms(*[c.reshape(-1) for c in cols])
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            if hierarchy:
                ctx.upload_hierarchy(parent, [0, 200, n])
            for _ in range(2):
                ctx.propagate_and_cull(frusta, flags=WHOLE)
            assert ctx.debug_scale_summary_uniform_waves()[0] == 4  # the summary is what the next all-rows frame reads the scale from
        a.anim_upload_tracks(tracks, T, np.concatenate([Vt.reshape(-1), S.reshape(-1)]))
        a.anim_upload_targets(targets)
        for seeks in ([0.3], [0.8], None):  # the scale animates, goes back to ONE, and a quiet frame
            if seeks:
                a.anim_frame(seeks)
                b.upload_transforms_indexed(*step_rows(cols, targets, per, seeks))
            for ctx in (a, b):
                ctx.propagate_and_cull(frusta, flags=WHOLE)
            g = same_state(a, b, cols, seeks)
            assert np.array_equal(g[row, [0, 4, 8]], cols[2][row]) and np.array_equal(cols[2][row], S[0] if seeks == [0.3] else S[1])
            assert a.debug_scale_summary_uniform_waves()[1].tobytes() == b.debug_scale_summary_uniform_waves()[1].tobytes()


def test_big_tree_few_targets_and_several_writers_in_a_frame():
    """6000 rows under the static-scene rule, 3 targets.  mi_columns_resize (context.cpp) sizes a half of the tree marks at the capacity
    rounded up to 256 plus 256 bytes: at least 6400 bytes = 1600 words here, and launch_anim_frame asks for ceil(words / 1024) >= 2
    clearing workgroups against the targets' one -- the workgroups past n_target_wgs only clear.  Each frame has three writers:
    anim_frame, anim_frame at other seek times, an indexed upload of two other rows (the later ones find the marks in place)."""
    n = 6000
    rng = np.random.default_rng(9)
    parent = np.full(n, B.NO_PARENT, U32)  # 2000 roots, a child and a grandchild each
    parent[2000:] = np.arange(4000)
    tracks, times, values, targets, per = build(rng, 3, n, STEP, 3, "shared", rows=[7, 2500, 4100])
    r = rng.normal(size=(n, 4))
    cols = [rng.normal(0, 3, (n, 3)).astype(F32), (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32), np.ones((n, 3), F32)]
    frusta, flags = view_frustum(), WHOLE | B.CULL_STATIC_OPT
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            ctx.resize(n)
            ctx.upload_transforms(*[c.reshape(-1) for c in cols])
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            ctx.upload_hierarchy(parent, [0, 2000, 4000, n])
            ctx.propagate_and_cull(frusta, flags=flags)
        a.anim_upload_tracks(tracks, times, values)
        a.anim_upload_targets(targets)
        for first, second, others in (([0.3, 0.6], [0.6, 0.3], [1999, 5999]), ([0.8, 0.3], [0.3, 0.8], [0, 4101]), ([0.6, 0.6], [0.8, 0.8], [2000, 3000]), (None, None, None)):  # (the last frame is quiet)
            if first:
                for seeks in (first, second):
                    a.anim_frame(seeks)
                    b.upload_transforms_indexed(*step_rows(cols, targets, per, seeks))
                cols[0][others] += F32(1)
                for ctx in (a, b):
                    ctx.upload_transforms_indexed(*rows_of(cols, others))
            for ctx in (a, b):
                ctx.propagate_and_cull(frusta, flags=flags | B.CULL_CHANGED_ROWS)
            same_state(a, b, cols, first)


def test_upload_life_cycle():
    """Targets uploaded three times (5, 300, 2: the count grows and shrinks), each serving frames; the tracks uploaded again drop the
    targets (MI_ERR_NOT_READY) until they come again."""
    n = 340
    rng = np.random.default_rng(13)
    tracks, times, values, targets, per = build(rng, 300, n, STEP, 3, "mixed")
    cols = [rng.normal(0, 3, (n, 3)).astype(F32), quat_keys(rng, n, 0), np.ones((n, 3), F32)]
    frusta, flags = view_frustum(), WHOLE | B.CULL_CHANGED_ROWS
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            ctx.resize(n)
            ctx.upload_transforms(*[c.reshape(-1) for c in cols])
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            ctx.propagate_and_cull(frusta, flags=WHOLE)
        a.anim_upload_tracks(tracks, times, values)

        def frames(pick, what):
            for seeks in ([0.3, 0.6], [0.8, 0.6]):
                a.anim_frame(seeks)
                b.upload_transforms_indexed(*step_rows(cols, targets[pick], [per[i] for i in pick], seeks))
                for ctx in (a, b):
                    ctx.propagate_and_cull(frusta, flags=flags)
                same_state(a, b, cols, (what, seeks))

        for pick in (np.arange(5), np.arange(300), np.array([7, 200])):
            a.anim_upload_targets(targets[pick])
            frames(pick, len(pick))
        a.anim_upload_tracks(tracks, times, values)
        with pytest.raises(B.MiError) as e:
            a.anim_frame([0.5, 0.5])
        assert e.value.code == api.MI_ERR_NOT_READY
        a.anim_upload_targets(targets[100:110])
        frames(np.arange(100, 110), "after the tracks came again")
        for ctx in (a, b):
            ctx.propagate_and_cull(frusta, flags=flags)
        same_state(a, b, cols, "quiet")


# ---- a rig through the whole frame: anim_frame -> propagate -> skin_frame
from test_gpu_skinning import bounds_ref, m3v, mat_ref, values as skin_values  # noqa: E402

EXACT_QUATS = np.array(list(np.eye(4)) + [[a, b, c, d] for a in (0.5, -0.5) for b in (0.5, -0.5) for c in (0.5, -0.5) for d in (0.5, -0.5)], F32)


def rigs(rng, interp, exact):
    """Two rigs of 20 joints (a root, a chain of three below it, four leaves under each of the four) and a mesh row each; a player per rig,
    a (t, r, s) track triple per joint over three shared key times.  exact: rotations whose matrices are exact in float32 (the unit
    axes and (+-1/2, +-1/2, +-1/2, +-1/2)), power-of-two scales, small integers elsewhere: every intermediate of the frame is
    representable.  Rows: roots 0 / 1, meshes 2 / 3, then level by level."""
    parent, joints, chain, levels = [B.NO_PARENT] * 4, [[0], [1]], [0, 1], [0, 4]
    for lvl in range(1, 5):
        nxt = []
        for r in range(2):
            first, k = len(parent), 5 if lvl < 4 else 4  # (the first child carries the chain on, until it ends)
            parent += [chain[r]] * k
            joints[r] += range(first, first + k)
            nxt.append(first)
        chain = nxt
        levels.append(len(parent))
    n, joints, T = len(parent), np.array(joints), np.array([0.25, 0.5, 0.75], F32)

    def vals(c, k):
        if c == 1:
            return EXACT_QUATS[rng.integers(0, 20, k)] if exact else quat_keys(rng, k, int(rng.integers(4)))
        if exact:
            return (rng.integers(-3, 4, (k, 3)) if c == 0 else 2.0 ** rng.integers(-1, 2, (k, 3))).astype(F32)
        return (rng.normal(0, 2, (k, 3)) if c == 0 else rng.uniform(0.5, 2, (k, 3))).astype(F32)

    cols = [vals(c, n) for c in range(3)]
    tracks, values, per, idx = [], [], [], []
    for j in joints.reshape(-1):
        tv = []
        for c in range(3):
            V = vals(c, 3)
            if interp == CUBIC:
                V = np.stack([rng.normal(0, 0.3, V.shape).astype(F32), V, rng.normal(0, 0.3, V.shape).astype(F32)], axis=1)
            tracks.append((0, 3, sum(map(len, values)), COMPS[c] | interp)), values.append(V.reshape(-1)), tv.append((T, V, interp))
        per.append(tv), idx.append([len(tracks) - 3, len(tracks) - 2, len(tracks) - 1])
    targets = targets_of(joints.reshape(-1), np.repeat([0, 1], 20), *np.array(idx, U32).T)
    skins = np.array([[2 + r, 20 * r, 20, 20 * r, 20 * r, 20] for r in range(2)], U32)
    fam = "exact" if exact else "random"
    skin = dict(pool=skin_values(rng, (40, 16), fam), skins=skins, a_joint=np.concatenate([rng.permutation(20) for _ in range(2)]).astype(U32),
                a_c=skin_values(rng, (40, 3), fam), a_h=np.abs(skin_values(rng, (40, 3), fam)))
    return dict(n=n, parent=np.array(parent, U32), levels=levels, joints=joints, cols=cols, tracks=np.array(tracks, B.ANIM_TRACK_DTYPE), times=T,
                values=np.concatenate(values), targets=targets, per=per, **skin)


def rig_context(ctx, rig):
    ctx.resize(rig["n"])
    ctx.upload_transforms(*[c.reshape(-1) for c in rig["cols"]])
    ctx.upload_bounds(np.zeros(3 * rig["n"], F32), np.ones(3 * rig["n"], F32))
    ctx.upload_hierarchy(rig["parent"], rig["levels"])
    ctx.upload_inverse_bindposes(rig["pool"])
    ctx.upload_skins(rig["skins"], rig["joints"].reshape(-1), rig["a_joint"], rig["a_c"], rig["a_h"])
    ctx.propagate()


def rig_outputs(ctx, flags=0):
    ctx.propagate(flags)
    ctx.skin_frame()
    return (ctx.download_global_transforms()[0].reshape(-1, 12), ctx.download_joint_matrices(), *ctx.download_skin_bounds(),
            ctx.download_changed_global_transforms()[0])


def rig_reference(rig, cols):
    """float64: Transform -> local affine (glam's Mat3::from_quat times the scale), parent * child down the levels, then the skinning
    test's mat_ref / bounds_ref -> GlobalTransforms [n, 12], joint matrices [40, 16], skin centers and half extents [2, 3]"""
    t, (x, y, z, w), s = cols[0].astype(F64), cols[1].astype(F64).T, cols[2].astype(F64)
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz, wx, wy, wz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2, w * x2, w * y2, w * z2
    g = np.stack([np.stack([1 - (yy + zz), xy + wz, xz - wy], 1) * s[:, 0:1], np.stack([xy - wz, 1 - (xx + zz), yz + wx], 1) * s[:, 1:2],
                  np.stack([xz + wy, yz - wx, 1 - (xx + yy)], 1) * s[:, 2:3], t], axis=1)  # [n, 4, 3]
    for i, p in enumerate(rig["parent"]):  # (parents come before their children)
        if p != B.NO_PARENT:
            g[i] = np.stack([*[m3v(g[p, :3], g[i, c]) for c in range(3)], m3v(g[p, :3], g[i, 3]) + g[p, 3]])
    g = g.reshape(-1, 12)
    rows = rig["joints"].reshape(-1)
    bounds = [bounds_ref(g, sk[0], rows[sk[1] + rig["a_joint"][sk[4]:sk[4] + sk[5]]], rig["a_c"][sk[4]:sk[4] + sk[5]], rig["a_h"][sk[4]:sk[4] + sk[5]], F64)
              for sk in rig["skins"]]
    return g, mat_ref(g[rows], rig["pool"], F64), np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds])


@pytest.mark.parametrize("interp,seeks", [(STEP, ([0.3, 0.6], [0.3, 0.8], [0.3, 0.4])), (LINEAR, ([0.25, 0.5], [0.25, 0.75], [0.25, 0.25]))],
                         ids=["step", "linear_on_keys"])
@pytest.mark.parametrize("static_opt", [False, True])
def test_rig_through_the_frame_exact(static_opt, interp, seeks):
    """Inputs for which every intermediate is representable: GlobalTransforms, joint matrices and refitted Aabbs equal a float64
    evaluation exactly.  Frame 2 moves rig 1 alone: rig 0's outputs keep their bits, and the changed-row list holds rig 1's joints and
    rig 0's root -- anim_frame stamps every target; a stamped root is assigned (its change tick moves), a stamped row below a root is
    set_if_neq(parent * local) and rig 0's compare equal.  Frame 3: rig 1's targets alone are uploaded and it moves again; the list
    holds rig 1's joints only under the static-scene rule, and rig 0's root as well without it (there the reference assigns every
    root that has children in every frame)."""
    rig = rigs(np.random.default_rng(21 + interp), interp, True)
    cols, outs = [c.copy() for c in rig["cols"]], []
    with B.Context() as ctx:
        rig_context(ctx, rig)
        ctx.anim_upload_tracks(rig["tracks"], rig["times"], rig["values"])
        ctx.anim_upload_targets(rig["targets"])
        for f, sk in enumerate(seeks):
            pick = np.arange(40) if f < 2 else np.arange(20, 40)
            if f == 2:
                ctx.anim_upload_targets(rig["targets"][pick])
            ctx.anim_frame(sk)
            want, bound = expected(cols, rig["targets"][pick], [rig["per"][i] for i in pick], np.array(sk, F32))
            assert not any(b.any() for b in bound)
            cols = [w.astype(F32) for w in want]
            outs.append(rig_outputs(ctx, B.PROPAGATE_STATIC_OPT if static_opt else 0))
            assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(ctx), cols))
            for got, ref in zip(outs[-1][:4], rig_reference(rig, cols)):
                assert np.array_equal(got.astype(F64), ref), f
            moved_and_root = np.concatenate([rig["joints"][0, :1], rig["joints"][1]])
            listed = rig["joints"].reshape(-1) if f == 0 else rig["joints"][1] if f == 2 and static_opt else moved_and_root
            assert np.array_equal(outs[-1][4], np.sort(listed)), f
    own = [rig["joints"][0], slice(0, 20), slice(0, 1), slice(0, 1)]  # rig 0 in: GlobalTransforms, joint matrices, centers, half extents
    for later in outs[1:]:
        assert all(later[i][own[i]].tobytes() == outs[0][i][own[i]].tobytes() for i in range(4))
    assert not np.array_equal(outs[1][1][20:], outs[0][1][20:]) and not np.array_equal(outs[2][1][20:], outs[1][1][20:])  # rig 1 did move


@pytest.mark.parametrize("interp", [LINEAR, CUBIC])
def test_rig_through_the_frame_against_an_upload_of_its_columns(interp):
    """Interpolated tracks need no tolerance downstream: the sampled columns, read back and handed to a twin as an indexed upload, must
    give the same GlobalTransforms, joint matrices, Aabbs and changed rows bit for bit."""
    rig = rigs(np.random.default_rng(31 + interp), interp, False)
    rows = rig["joints"].reshape(-1)
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            rig_context(ctx, rig)
        a.anim_upload_tracks(rig["tracks"], rig["times"], rig["values"])
        a.anim_upload_targets(rig["targets"])
        for sk in ([0.3, 0.6180339], [0.3, 0.7]):
            a.anim_frame(sk)
            cols = read_columns(a)
            b.upload_transforms_indexed(*rows_of(cols, rows))
            for x, y in zip(rig_outputs(a), rig_outputs(b)):
                assert x.tobytes() == y.tobytes() and len(x)
