"""mi_anim_frame_blended (weighted clip layers folded into Transforms on the device) against `blend` below: test_gpu_animation's float64
`sample` per layer, folded by the rule include/bevy_mi355x.h states (first contributing layer taken as it is; a later one moves the
accumulator by u = weight / (weights so far + weight); lerp for translation and scale, the header's slerp for rotation).
Bounds, e = 2^-24:
  unwritten components, rows of players without kept layers, single contributors   what `sample` allows: bit for bit, or its own bound
  blended translation / scale   the samples' own bounds + 8 e (|acc| + |v|) per fold step (two roundings of u, three of the lerp)
  blended rotations             ROT_BOUND = 17 e per component: four times the 4.27 e a float32 run of this reference deviates from its float64
      run over all the cases below (tools/probes/animation_probe.py --blend-deviation); every fold step keeps |dot| > 1e-3 and ||dot| - 0.9995| > 1e-4
Measured on an MI355X (profiles/r11_blend/ab.md): the worst error of any case, blended rotations included, is 0.25 of its bound."""
import functools

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api
from test_gpu_animation import COMPS, CUBIC, E, F32, F64, LINEAR, STEP, U32, WHOLE, compare, key_times, read_columns, sample, targets_of, view_frustum

pytestmark = pytest.mark.gpu

NO, CLIPS = B.ANIM_NO_TRACK, 8
ROT_BOUND = 17 * E


def blend(layers, rot, dt=F64):
    """One component of one target: layers = [(T, V, interp, x, weight)], kept and contributing, in blend order -> (value, bound)"""
    acc = None
    for T, V, interp, x, wt in layers:
        v, b = sample(T, V, rot, interp, x, dt)
        if acc is None:
            acc, wsum, bound = v, dt(wt), b
            continue
        wsum = wsum + dt(wt)
        u = dt(wt) / wsum
        if not rot:
            bound = bound + b + 8 * E * (abs(acc) + abs(v))
            acc = acc + (v - acc) * u
            continue
        dot = (acc[0] * v[0] + acc[2] * v[2]) + (acc[1] * v[1] + acc[3] * v[3])
        assert abs(dot) > 1e-3 and abs(abs(dot) - 0.9995) > 1e-4, dot  # the slerp's branches are decidable
        if dot < 0:
            v, dot = -v, -dot
        if dot > dt(0.9995):
            q = acc + (v - acc) * u
            acc = q / np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
        else:
            th = np.arccos(dot)
            acc = (acc * np.sin(th * (1 - u)) + v * np.sin(th * u)) * (1 / np.sin(th))
        bound = ROT_BOUND
    return acc, bound


def scene(seed, groups, interp_of=lambda c: c % 3, dropped=False):
    """Player p has groups[p] = (targets, kept layers); every target binds CLIPS clips, clip c's tracks of interpolation interp_of(c) over
    four key times of the clip's own.  A fifth of the (target, clip, component) bindings have no track; in the players behind the first,
    target 1 has no scale track in any clip and target 2 no track at all.  Rotations of a target lie 0.3 .. 0.9 (every fourth target:
    2e-3 and small tangents, the slerp's nlerp branch) off a base of its own, with random signs.  Weights 1e-3 .. 1e3, the first seek time a key.
    dropped: layers of weight 0, -1 and NaN among the first player's."""
    rng = np.random.default_rng(seed)
    n = sum(g[0] for g in groups)
    T = [key_times(rng, 4) for _ in range(CLIPS)]
    tracks, values, per, n_v = [], [], [], 0
    players = np.repeat(np.arange(len(groups)), [g[0] for g in groups])
    index = np.concatenate([np.arange(g[0]) for g in groups])
    bindings = np.full(n * CLIPS, NO, B.ANIM_BINDING_DTYPE)
    for i in range(n):
        base, reach, tv = rng.normal(size=4), (2e-3, 2e-3) if i % 4 == 3 else (0.3, 0.9), []
        for c in range(CLIPS):
            tv.append([None] * 3)
            for k in range(3):
                if (i + 2 * c + k) % 5 == 0 or (players[i] and (index[i] == 2 or (index[i] == 1 and k == 2))):
                    continue
                V = rng.normal(0, 2, (4, 4 if k == 1 else 3))
                if k == 1:
                    V -= np.outer(V @ base, base) / (base @ base)
                    V = base / np.linalg.norm(base) + rng.uniform(*reach, (4, 1)) * V / np.linalg.norm(V, axis=1, keepdims=True)
                    V *= rng.choice([-1.0, 1.0], (4, 1)) / np.linalg.norm(V, axis=1, keepdims=True)
                V = V.astype(F32)
                if interp_of(c) == CUBIC:
                    tan = lambda: rng.normal(0, 0.03 if k == 1 and i % 4 == 3 else 0.3, V.shape).astype(F32)
                    V = np.stack([tan(), V, tan()], axis=1)
                bindings[i * CLIPS + c][k], tv[c][k] = len(tracks), (T[c], V, interp_of(c))
                tracks.append((4 * c, 4, n_v, COMPS[k] | interp_of(c)))
                values.append(V.reshape(-1))
                n_v += V.size
        per.append(tv)
    kept, layers = [], []
    for p, (_, n_layers) in enumerate(groups):
        wt = (10.0 ** rng.uniform(-3, 3, n_layers)).astype(F32)
        wt[:1], wt[1:][-1:] = 1e-3, 1e3
        kept.append(list(zip(rng.permutation(CLIPS)[:n_layers], np.r_[0.5, rng.uniform(0.2, 0.8, CLIPS)].astype(F32), wt)))
        layers += [(p, *ly) for ly in kept[-1]]
        if dropped and p == 0:
            layers[:0], layers[len(layers) // 2:len(layers) // 2] = [(0, 1, 0.4, 0.0)], [(0, 2, 0.4, -1.0)]
            layers.append((0, 3, 0.4, np.nan))
    n_rows = n + 40
    tg = np.zeros(n, B.ANIM_BLEND_TARGET_DTYPE)
    tg["row"], tg["player"], tg["first_binding"], tg["n_clips"] = rng.permutation(n_rows)[:n], players, CLIPS * np.arange(n), CLIPS
    return dict(n=n_rows, tracks=np.array(tracks, B.ANIM_TRACK_DTYPE), times=np.concatenate(T), values=np.concatenate(values), targets=tg,
                bindings=bindings, layers=np.array(layers, B.ANIM_LAYER_DTYPE), kept=kept, per=per, players=len(groups),
                cur=[rng.normal(0, 1, (n_rows, w)).astype(F32) for w in (3, 4, 3)], written=np.sort(tg["row"][[bool(kept[p]) for p in players]]))


def expected(sc, cur, dt=F64):
    want, bound = [c.astype(dt) for c in cur], [np.zeros(c.shape) for c in cur]
    for tg, tv in zip(sc["targets"], sc["per"]):
        for k in range(3):
            ls = [(*tv[c][k], x, wt) for c, x, wt in sc["kept"][tg["player"]] if tv[c][k] is not None]
            if ls:
                want[k][tg["row"]], bound[k][tg["row"]] = blend(ls, k == 1, dt)
    return want, bound


def start(ctx, sc, upload=True):
    ctx.resize(sc["n"])
    ctx.upload_transforms(*[c.reshape(-1) for c in sc["cur"]])
    ctx.propagate()  # (consumes the rows' Added<GlobalTransform>)
    if upload:
        ctx.anim_upload_tracks(sc["tracks"], sc["times"], sc["values"])
        ctx.anim_upload_blend_targets(sc["targets"], sc["bindings"])


# the workgroup seam (64 targets) and the round seam (4 layers); behind the swept player three more, of 1, 5 and 0 layers
CASES = sorted({(65, L) for L in (1, 2, 4, 5, 8)} | {(n, L) for n in (1, 63, 64, 65, 129) for L in (4, 5)})


def blend_scene(n, L):
    return scene(1000 * n + L, [(n, L), (3, 1), (3, 5), (3, 0)], dropped=True)


@pytest.mark.parametrize("n,L", CASES)
def test_blend_against_float64(n, L):
    sc = blend_scene(n, L)
    want, bound = expected(sc, sc["cur"])
    assert (bound[1] == ROT_BOUND).any()
    with B.Context() as ctx:
        start(ctx, sc)
        ctx.anim_frame_blended(sc["players"], sc["layers"])
        compare(read_columns(ctx), want, bound, f"{n} targets, {L} layers")
        ctx.propagate(0)
        assert np.array_equal(ctx.download_changed_global_transforms()[0], sc["written"])  # (the targets of the 0-layer player are not among them)


@pytest.mark.parametrize("weight", [1e-3, 1, 7])
@pytest.mark.parametrize("interp", [STEP, LINEAR, CUBIC])
def test_one_layer_is_anim_frame(interp, weight):
    sc = scene(50 + interp, [(70, 1), (30, 1)], interp_of=lambda c: interp)
    clip = np.array([sc["kept"][p][0][0] for p in sc["targets"]["player"]])
    single = targets_of(sc["targets"]["row"], sc["targets"]["player"], *[sc["bindings"][CLIPS * np.arange(100) + clip][f] for f in ("track_t", "track_r", "track_s")])
    layers = sc["layers"].copy()
    layers["weight"] = weight
    with B.Context() as a, B.Context() as b:
        start(a, sc), start(b, sc)
        a.anim_upload_targets(single)
        a.anim_frame(layers["seek_time"])
        b.anim_frame_blended(2, layers)
        got = read_columns(b)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(a), got)) and not np.array_equal(got[1], sc["cur"][1])


@pytest.mark.parametrize("static", [True, False])
@pytest.mark.parametrize("hierarchy", [True, False])
def test_state_equals_an_indexed_upload(hierarchy, static):
    """Against an indexed upload of the columns it produced, on a twin context, over two frames; the middle player has no layers."""
    sc = scene(7, [(60, 2), (40, 0), (60, 5)])
    n = sc["n"]
    parent = np.full(n, B.NO_PARENT, U32)  # level 0: rows [0, 100), twenty of them with children; level 1: [100, 150); level 2: [150, n)
    parent[100:150], parent[150:] = np.arange(50) // 5 * 5, 100 + np.arange(n - 150) % 50
    frusta, flags = view_frustum(), WHOLE | (B.CULL_STATIC_OPT if static else 0)
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            start(ctx, sc, upload=ctx is a)
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            if hierarchy:
                ctx.upload_hierarchy(parent, [0, 100, 150, n])
            ctx.propagate_and_cull(frusta, flags=flags)
        for frame in range(2):
            layers = sc["layers"][::1 + frame]  # (the second frame: every other layer, at other weights)
            a.anim_frame_blended(3, layers)
            cols = read_columns(a)
            b.upload_transforms_indexed(sc["written"], *[c[sc["written"]].reshape(-1) for c in cols])
            for ctx in (a, b):
                ctx.propagate_and_cull(frusta, flags=flags | B.CULL_CHANGED_ROWS)
            (ga, ca), (gb, cb) = a.download_global_transforms(), b.download_global_transforms()
            assert ga.tobytes() == gb.tobytes() and np.array_equal(ca, cb) and np.array_equal(a.download_visibility(0), b.download_visibility(0))
            assert np.array_equal(a.download_changed_global_transforms()[0], b.download_changed_global_transforms()[0])
            assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(b), cols))


def frame(ctx, sc, **changes):
    layers = sc["layers"].copy()
    for field, (at, value) in changes.items():
        layers[field][at] = value
    ctx.anim_frame_blended(2, layers)


def upload(ctx, sc, **changes):
    tg, bd = sc["targets"].copy(), sc["bindings"].copy()
    for field, (at, value) in changes.items():
        (tg if field in tg.dtype.names else bd)[field][at] = value
    ctx.anim_upload_blend_targets(tg, bd)


BAD = {  # name -> (the refused call, its error); the scene: players 0 and 1 with 4 layers each, layers 0..3 and 4..7
    "layers out of player order": (lambda ctx, sc: frame(ctx, sc, player=(0, 1)), api.MI_ERR_INVALID_ARG),
    "clip >= n_clips": (lambda ctx, sc: frame(ctx, sc, clip=(5, CLIPS)), api.MI_ERR_INVALID_ARG),
    "nine kept layers": (lambda ctx, sc: ctx.anim_frame_blended(2, np.concatenate([sc["layers"][:4]] * 2 + [sc["layers"][:1], sc["layers"][4:]])), api.MI_ERR_INVALID_ARG),
    "a player >= n_players": (lambda ctx, sc: frame(ctx, sc, player=(7, 2)), api.MI_ERR_INVALID_ARG),
    "duplicate rows": (lambda ctx, sc: upload(ctx, sc, row=(1, sc["targets"]["row"][0])), api.MI_ERR_INVALID_ARG),
    "a binding range past the array": (lambda ctx, sc: upload(ctx, sc, first_binding=(3, len(sc["bindings"]) - CLIPS + 1)), api.MI_ERR_INVALID_ARG),
    "a rotation track in track_t": (lambda ctx, sc: upload(ctx, sc, track_t=(0, sc["bindings"]["track_r"][1])), api.MI_ERR_INVALID_ARG),
    "a frame before the uploads": (None, api.MI_ERR_NOT_READY),
    "a frame after the tracks dropped the targets": (lambda ctx, sc: (ctx.anim_upload_tracks(sc["tracks"], sc["times"], sc["values"]), frame(ctx, sc)), api.MI_ERR_NOT_READY),
}


@functools.lru_cache(None)
def good_frame():
    sc = scene(3, [(5, 4), (4, 4)])
    with B.Context() as ctx:
        start(ctx, sc)
        frame(ctx, sc)
        return sc, read_columns(ctx)


@pytest.mark.parametrize("what", list(BAD))
def test_argument_checks(what):
    (sc, good), (call, code) = good_frame(), BAD[what]
    with B.Context() as ctx:
        start(ctx, sc, upload=False)
        with pytest.raises(B.MiError) as e:
            if call is None:
                frame(ctx, sc)
            ctx.anim_upload_tracks(sc["tracks"], sc["times"], sc["values"])
            upload(ctx, sc)
            call(ctx, sc)
        assert e.value.code == code
        if code == api.MI_ERR_NOT_READY:  # (the uploads are made now where there were none, or none any more)
            start(ctx, sc)
        frame(ctx, sc)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(ctx), good))
