"""mi_anim_frame_weights (weight tracks, n floats per key, run through animation graphs into an array of morph weights on the device)
against `evaluate` below: a float64 restatement of the rules include/bevy_mi355x.h states, each weight a scalar sampled by
test_gpu_animation's `sample` as a translation component is.  Bounds, e = 2^-24: the sampling's own (8 e (|a| + |b|) LINEAR, 24 e S CUBIC,
derived at the head of test_gpu_animation.py), + 8 e (|acc| + |v|) per BLEND step and b_acc + |w| b_v + 4 e (|acc| + |v w|) per ADD step
(test_gpu_anim_graph.py).  STEP values, first / last / on-key samples, single present clips and every weight nothing writes: bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api
from test_gpu_animation import CUBIC, E, F32, F64, LINEAR, STEP, U32, read_columns, sample
from test_gpu_anim_graph import SHAPES, graph_arrays

pytestmark = pytest.mark.gpu

NO, CLIP, BLEND, ADD = B.ANIM_NO_NODE, B.ANIM_NODE_CLIP, B.ANIM_NODE_BLEND, B.ANIM_NODE_ADD
NESTED = [(ADD, NO, 0), (BLEND, 0, 0), (BLEND, 1, 0), (CLIP, 2, 0), (CLIP, 2, 1), (CLIP, 1, 2), (CLIP, 0, 3)]  # add(blend(blend(c0,c1),c2),c3)
GRAPHS = {  # name -> (node table, {node: own mask}, {node: weight instead of a random one})
    "a root clip": ([(CLIP, NO, 0)], {}, {}),
    "blend of 2": ([(BLEND, NO, 0), (CLIP, 0, 0), (CLIP, 0, 1)], {}, {}),
    "blend of 5": ([(BLEND, NO, 0)] + [(CLIP, 0, c) for c in range(5)], {}, {}),
    "add(blend(blend(c0,c1),c2),c3)": (NESTED, {}, {}),
    "chain of 8": (SHAPES["chain of 8"], {}, {}),
    "a mask on an inner node, hitting one of a player's two targets": (NESTED, {2: 1}, {}),
    "an inner node of weight 0": (NESTED, {}, {2: 0.0}),
    "an inner node of weight -1": (NESTED, {}, {1: -1.0}),
    "a clip of weight NaN": (NESTED, {}, {5: np.nan}),
    "an absent root": (NESTED, {}, {0: 0.0}),
}


def evaluate(nodes, masks, k, st, tv, groups, eff=0):
    """One target: node k under the states st -> (its n weights, their bounds), or None = absent"""
    kind, _, clip = nodes[k]
    eff |= masks.get(k, 0)
    if not st["weight"][k] > 0 or eff & groups:
        return None
    if kind == CLIP:
        return None if tv[clip] is None else sample(tv[clip][0], tv[clip][1], False, tv[clip][2], st["seek_time"][k])
    acc = None
    for j in [j for j, nd in enumerate(nodes) if nd[1] == k]:
        r = evaluate(nodes, masks, j, st, tv, groups, eff)
        if r is None:
            continue
        (v, b), w = r, F64(st["weight"][j])
        if acc is None:
            acc, bound, wsum = v, b + 0 * v, w
        elif kind == BLEND:
            wsum = wsum + w
            acc, bound = acc + (v - acc) * (w / wsum), bound + b + 8 * E * (abs(acc) + abs(v))
        else:
            acc, bound = acc + v * w, bound + abs(w) * b + 4 * E * (abs(acc) + abs(v * w))
    return None if acc is None else (acc, bound)


def scene(seed, targets, name, k=4, interp_of=lambda c: c % 3, idle=(), unbound=(), gap=2, seeks=None):
    """targets: [(player, n_weights, groups)], each writing a range of its own with `gap` weights nothing writes behind it.  Every player
    runs GRAPHS[name]; clip slot c has k key times of its own and, per target, a track of interpolation interp_of(c) -- none where
    (target, c) is in unbound.  Node weights 1e-3 .. 1e3; seek times 0.2 .. 0.8, or seeks[player] for every node; idle: players left alone."""
    rng = np.random.default_rng(seed)
    nodes, masks, weights = GRAPHS[name]
    clips = 1 + max(nd[2] for nd in nodes)
    T = np.linspace(0.25, 0.75, k).astype(F32) if k > 1 else np.array([0.25], F32)  # (every clip the same k times, in a range of its own)
    tracks, values, per, bindings, n_v, n_out = [], [], [], [], 0, 0
    tg = np.zeros(len(targets), B.ANIM_MORPH_TARGET_DTYPE)
    for i, (p, n_w, groups) in enumerate(targets):
        per.append([])
        for c in range(clips):
            if (i, c) in unbound:
                per[-1].append(None), bindings.append(B.ANIM_NO_TRACK)
                continue
            V = rng.normal(0, 2, (k, 3, n_w) if interp_of(c) == CUBIC else (k, n_w)).astype(F32)
            per[-1].append((T, V, interp_of(c))), bindings.append(len(tracks))
            tracks.append((k * c, k, n_v, interp_of(c), n_w)), values.append(V.reshape(-1))
            n_v += V.size
        tg[i] = (p, n_out, n_w, i * clips, clips, groups & 0xFFFFFFFF, groups >> 32)
        n_out += n_w + gap
    n_players = 1 + max(t[0] for t in targets)
    states = np.zeros(n_players * len(nodes), B.ANIM_NODE_STATE_DTYPE)
    states["weight"], states["seek_time"] = 10.0 ** rng.uniform(-3, 3, len(states)), rng.uniform(0.2, 0.8, len(states))
    for p in range(n_players):
        for node, w in weights.items():
            states["weight"][p * len(nodes) + node] = w
        if seeks is not None:
            states["seek_time"][p * len(nodes):(p + 1) * len(nodes)] = seeks[p]
    return dict(tracks=np.array(tracks, B.ANIM_WEIGHT_TRACK_DTYPE), times=np.tile(T, clips), values=np.concatenate(values), targets=tg, bindings=np.array(bindings, U32),
                per=per, graphs=[nodes], masks={(0, k): m for k, m in masks.items()}, player_graph=np.zeros(n_players, U32), states=states,
                first_state=np.array([NO if p in idle else p * len(nodes) for p in range(n_players)], U32), initial=rng.normal(0, 1, n_out).astype(F32),
                groups=[t[2] for t in targets])


def expected(sc, cur):
    want, bound = cur.astype(F64), np.zeros(len(cur))
    nodes = sc["graphs"][0]
    for tg, tv, groups in zip(sc["targets"], sc["per"], sc["groups"]):
        first = sc["first_state"][tg["player"]]
        r = None if first == NO else evaluate(nodes, {k: m for (_, k), m in sc["masks"].items()}, 0, sc["states"][first:first + len(nodes)], tv, groups)
        if r is not None:
            want[tg["first_weight"]:tg["first_weight"] + tg["n_weights"]], bound[tg["first_weight"]:tg["first_weight"] + tg["n_weights"]] = r
    return want, bound


def load(ctx, sc):
    ctx.anim_upload_weight_tracks(sc["tracks"], sc["times"], sc["values"])
    ctx.anim_upload_graphs(*graph_arrays(sc))
    ctx.anim_upload_morph_targets(sc["targets"], sc["bindings"], sc["player_graph"], len(sc["initial"]), sc["initial"])


def frame(ctx, sc, **kw):
    ctx.anim_frame_weights(kw.get("first_state", sc["first_state"]), sc["states"])


def check(ctx, sc, cur, what):
    want, bound = expected(sc, cur)
    got, exact = ctx.anim_download_weights(), bound == 0  # (exact: the bit-for-bit cases, and every weight no target writes this frame)
    assert np.array_equal(got.view(U32)[exact], want.astype(F32).view(U32)[exact]), what
    err = np.abs(got - want)[~exact]
    print(f"{what}: max error / bound {np.max(err / bound[~exact], initial=0.0):.3f} over {err.size} weights")
    assert np.all(err <= bound[~exact]), what
    return got


SAMPLING = [(n_w, 65, i) for n_w in (1, 63, 64, 65, 130) for i in (STEP, LINEAR, CUBIC)] + [(65, k, i) for k in (1, 2, 64, 130) for i in (STEP, LINEAR, CUBIC)]
SAMPLING += [(1, 4097, i) for i in (STEP, LINEAR, CUBIC)]


@pytest.mark.parametrize("n_w,k,interp", SAMPLING)
def test_sampling_under_a_root_clip(n_w, k, interp):
    """Seven players, a target each, at: before the track, on key k // 2, one ulp below and above it, between keys, behind the track, NaN;
    an eighth left alone."""
    on = F32(np.linspace(0.25, 0.75, k).astype(F32)[k // 2] if k > 1 else 0.25)
    seeks = np.array([0.1, on, np.nextafter(on, F32(0)), np.nextafter(on, F32(1)), 0.6180339, 0.9, np.nan, 0.5], F32)
    sc = scene(100 * n_w + k, [(p, n_w, 0) for p in range(8)], "a root clip", k=k, interp_of=lambda c: interp, idle=(7,), seeks=seeks)
    with B.Context() as ctx:
        load(ctx, sc)
        frame(ctx, sc)
        check(ctx, sc, sc["initial"], f"{n_w} weights, {k} keys, interpolation {interp}")


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graphs_against_float64(name):
    """Player 0: targets of 65 and of 3 weights in different mask groups, the first without a track for clip slot 1; player 1: 130 weights;
    player 2 is left alone.  A second frame over what the first left: an absent root keeps it."""
    sc = scene(len(name), [(0, 65, 1), (0, 3, 2), (1, 130, 2), (2, 5, 1)], name, idle=(2,), unbound={(0, 1)})
    with B.Context() as ctx:
        load(ctx, sc)
        assert ctx.anim_download_weights().tobytes() == sc["initial"].tobytes() and ctx.device_buffer(api.BUF_MORPH_WEIGHTS)[1] == 4 * len(sc["initial"])
        frame(ctx, sc)
        cur = check(ctx, sc, sc["initial"], name)
        assert (cur.tobytes() == sc["initial"].tobytes()) == (name == "an absent root")
        sc["states"]["weight"][0], sc["states"]["seek_time"][:] = 0.0, 0.4  # player 0's root goes absent, player 1 moves on
        frame(ctx, sc)
        check(ctx, sc, cur, name + ", second frame")


def transform_side(ctx, sc, cur):
    """The same keys as translation tracks of rows 0 .. n (target i = row i = weights [3 i, 3 i + 3)), through mi_anim_upload_graph_targets"""
    tr = np.zeros(len(sc["tracks"]), B.ANIM_TRACK_DTYPE)
    for f in ("first_time", "n_keys", "first_value"):
        tr[f] = sc["tracks"][f]
    tr["kind_interp"] = B.ANIM_TRANSLATION | sc["tracks"]["interp"]
    bd = np.full(len(sc["bindings"]), B.ANIM_NO_TRACK, B.ANIM_BINDING_DTYPE)
    bd["track_t"] = sc["bindings"]
    tg = np.zeros(len(sc["targets"]), B.ANIM_GRAPH_TARGET_DTYPE)
    tg["row"] = np.arange(len(tg))
    for f in ("player", "first_binding", "n_clips"):
        tg[f] = sc["targets"][f]
    ctx.resize(len(tg))
    ctx.upload_transforms(*[c.reshape(-1) for c in cur])
    ctx.propagate()
    ctx.anim_upload_tracks(tr, sc["times"], sc["values"])
    ctx.anim_upload_graph_targets(tg, bd, sc["player_graph"])


@pytest.mark.parametrize("interp", [LINEAR, CUBIC])
@pytest.mark.parametrize("name", ["blend of 5", "add(blend(blend(c0,c1),c2),c3)"])
def test_three_weights_are_a_translation_bit_for_bit(name, interp):
    """... and a twin context that never hears of weights ends with the same Transform columns and changed rows."""
    sc = scene(11 + interp, [(i % 2, 3, 0) for i in range(70)], name, k=5, interp_of=lambda c: interp, gap=0, unbound={(3, 0)})
    cur = [np.random.default_rng(5).normal(0, 1, (70, w)).astype(F32) for w in (3, 4, 3)]
    sc["initial"] = cur[0].reshape(-1).copy()
    with B.Context() as a, B.Context() as b:
        load(a, sc)
        b.anim_upload_graphs(*graph_arrays(sc))
        for ctx in (a, b):
            transform_side(ctx, sc, cur)  # (behind the weights' uploads: mi_anim_upload_tracks leaves them alone, as theirs left it alone)
        frame(a, sc)
        for ctx in (a, b):
            ctx.anim_frame_graph(sc["first_state"], sc["states"])
        cols_a, cols_b = read_columns(a), read_columns(b)
        assert a.anim_download_weights().tobytes() == cols_a[0].tobytes() and not np.array_equal(cols_a[0], cur[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(cols_a, cols_b))
        for ctx in (a, b):
            ctx.propagate(0)
        assert np.array_equal(a.download_changed_global_transforms()[0], b.download_changed_global_transforms()[0])


def tracks_with(ctx, sc, field, at, value, times=None):
    tr = sc["tracks"].copy()
    tr[field][at] = value
    ctx.anim_upload_weight_tracks(tr, sc["times"] if times is None else times, sc["values"])


def targets_with(ctx, sc, player_graph=None, bindings=None, n_out=None, **changes):
    tg, bd = sc["targets"].copy(), sc["bindings"].copy()
    for field, (at, value) in changes.items():
        tg[field][at] = value
    for at, value in (bindings or {}).items():
        bd[at] = value
    ctx.anim_upload_morph_targets(tg, bd, sc["player_graph"] if player_graph is None else player_graph, len(sc["initial"]) if n_out is None else n_out)


def raw_frame(ctx, sc, flags):
    fs, st = sc["first_state"], sc["states"]
    ctx._ck(ctx._lib.mi_anim_frame_weights(ctx._h, len(fs), fs.ctypes.data_as(C.c_void_p), len(st), st.ctypes.data_as(C.c_void_p), C.c_uint32(flags)))


INVALID, NOT_READY = api.MI_ERR_INVALID_ARG, api.MI_ERR_NOT_READY
BAD = {  # name -> (the refused call, its error); the scene: NESTED (clip slots 0 .. 3) over targets of 65 + 3 weights (player 0) and 5 (player 1)
    "times outside the pool": (lambda ctx, sc: tracks_with(ctx, sc, "first_time", 1, len(sc["times"]) - 3), INVALID),
    "values outside the pool": (lambda ctx, sc: tracks_with(ctx, sc, "first_value", 1, len(sc["values"]) - 4 * 65 + 1), INVALID),
    "a track without keys": (lambda ctx, sc: tracks_with(ctx, sc, "n_keys", 0, 0), INVALID),
    "a track without weights": (lambda ctx, sc: tracks_with(ctx, sc, "n_weights", 0, 0), INVALID),
    "an unknown interpolation": (lambda ctx, sc: tracks_with(ctx, sc, "interp", 0, 3), INVALID),
    "times that do not ascend": (lambda ctx, sc: tracks_with(ctx, sc, "interp", 0, 0, times=np.r_[sc["times"][:2], sc["times"][1:-1]]), INVALID),
    "an output range past the array": (lambda ctx, sc: targets_with(ctx, sc, n_out=len(sc["initial"]) - 3), INVALID),
    "output ranges that overlap": (lambda ctx, sc: targets_with(ctx, sc, first_weight=(2, 66)), INVALID),
    "a target without weights": (lambda ctx, sc: targets_with(ctx, sc, n_weights=(1, 0)), INVALID),
    "a target without clips": (lambda ctx, sc: targets_with(ctx, sc, n_clips=(1, 0)), INVALID),
    "a binding range past the array": (lambda ctx, sc: targets_with(ctx, sc, first_binding=(2, 9)), INVALID),
    "a track that does not exist": (lambda ctx, sc: targets_with(ctx, sc, bindings={5: len(sc["tracks"])}), INVALID),
    "a track of another width": (lambda ctx, sc: targets_with(ctx, sc, bindings={5: 0}), INVALID),
    "a target's player >= n_players": (lambda ctx, sc: targets_with(ctx, sc, player=(0, 2)), INVALID),
    "a graph that does not exist": (lambda ctx, sc: targets_with(ctx, sc, player_graph=[0, 1]), INVALID),
    "targets of a player without a graph": (lambda ctx, sc: targets_with(ctx, sc, player_graph=[0, NO]), INVALID),
    "a clip node's clip >= n_clips": (lambda ctx, sc: targets_with(ctx, sc, n_clips=(1, 3)), INVALID),
    "states past the array": (lambda ctx, sc: frame(ctx, sc, first_state=[0, 8]), INVALID),
    "states for a player without a graph": (lambda ctx, sc: frame(ctx, sc, first_state=[0, 7, 0]), INVALID),
    "fewer players than the targets name": (lambda ctx, sc: frame(ctx, sc, first_state=[0]), INVALID),
    "nonzero flags": (lambda ctx, sc: raw_frame(ctx, sc, 1), INVALID),
    "a frame before the uploads": (None, NOT_READY),
    "morph targets before the weight tracks": (None, NOT_READY),
    "a frame after the graphs dropped the targets": (lambda ctx, sc: (ctx.anim_upload_graphs(*graph_arrays(sc)), frame(ctx, sc)), NOT_READY),
    "a frame after the weight tracks dropped the targets": (lambda ctx, sc: (ctx.anim_upload_weight_tracks(sc["tracks"], sc["times"], sc["values"]), frame(ctx, sc)), NOT_READY),
}


@functools.lru_cache(None)
def good_frame():
    sc = scene(3, [(0, 65, 1), (0, 3, 2), (1, 5, 2)], "add(blend(blend(c0,c1),c2),c3)")
    with B.Context() as ctx:
        load(ctx, sc)
        frame(ctx, sc)
        return sc, ctx.anim_download_weights()


@pytest.mark.parametrize("what", list(BAD))
def test_argument_checks(what):
    (sc, good), (call, code) = good_frame(), BAD[what]
    with B.Context() as ctx:
        if call is not None:
            load(ctx, sc)
        elif what.startswith("morph targets"):
            ctx.anim_upload_graphs(*graph_arrays(sc))
            call = targets_with
        with pytest.raises(B.MiError) as e:
            (call or frame)(ctx, sc)
        assert e.value.code == code
        if code == NOT_READY:  # (the uploads are made now where there were none, or none any more)
            load(ctx, sc)
        frame(ctx, sc)
        assert ctx.anim_download_weights().tobytes() == good.tobytes()
