"""mi_anim_frame_graph (a tree of CLIP / BLEND / ADD nodes with weights and masks, evaluated per target on the device) against
`evaluate` below: a float64 restatement of the rules include/bevy_mi355x.h states, over test_gpu_animation's `sample` and
test_gpu_anim_blend's `scene` (STEP / LINEAR / CUBIC tracks, a fifth of the bindings without a track, weights 1e-3 .. 1e3).
Bounds, e = 2^-24:
  absent components, rows of players left alone, a single present clip   what `sample` allows: bit for bit, or its own bound
  translation / scale   the samples' own bounds + 8 e (|acc| + |v|) per BLEND step; per ADD step b_acc + |w| b_v + 4 e (|acc| + |v w|)
  folded rotations      per shape, ROT_BOUND: four times what a float32 run of this reference deviates from its float64 run over the
      nested and the mask cases below (tools/probes/animation_probe.py --graph-deviation, no GPU): ROT_DEVIATION.  An additive clip
      of weight ~1e3 turns th * w into an angle of hundreds of radians, which float32 holds to ~1e-5, and an ADD node over an inner
      node multiplies that node's own error by its weight: hence the size of those numbers (the chain of 8 stacks three ADD levels and
      its rotation bound, 0.49, says little; its translations, scales and absent components are held as tightly as everywhere).
      Every slerp, additive ones included, keeps |dot| > 1e-3 and ||dot| - 0.9995| > 1e-4 (asserted; SEEDS are chosen so that it holds).
Measured on an MI355X (profiles/r12_graph/ab.md): the worst error of any bounded comparison is 0.45 of its bound."""
import functools

import numpy as np
import pytest

import bevy_amd as B
from bevy_amd import api
from test_gpu_animation import E, F32, F64, U32, WHOLE, compare, read_columns, sample, targets_of, view_frustum
from test_gpu_anim_blend import CLIPS, scene, start

pytestmark = pytest.mark.gpu

NO, CLIP, BLEND, ADD = B.ANIM_NO_NODE, B.ANIM_NODE_CLIP, B.ANIM_NODE_BLEND, B.ANIM_NODE_ADD
SHAPES = {  # node tables: (kind, parent, clip slot)
    "blend(blend(c0,c1),c2)": [(BLEND, NO, 0), (BLEND, 0, 0), (CLIP, 1, 0), (CLIP, 1, 1), (CLIP, 0, 2)],
    "add(blend(c0,c1),c2)": [(ADD, NO, 0), (BLEND, 0, 0), (CLIP, 1, 0), (CLIP, 1, 1), (CLIP, 0, 2)],
    "blend(add(c0,c1),blend(c2,add(c3,c4)),c5)": [(BLEND, NO, 0), (ADD, 0, 0), (CLIP, 1, 0), (CLIP, 1, 1), (BLEND, 0, 0), (CLIP, 4, 2), (ADD, 4, 0), (CLIP, 6, 3),
                                                  (CLIP, 6, 4), (CLIP, 0, 5)],
    # depth 8: inner node 2 j at depth j + 1 (BLEND, ADD, BLEND, ...) holds clip j and the next inner node; clip 7 at depth 8
    "chain of 8": [nd for j in range(7) for nd in ((BLEND + j % 2, 2 * j - 2 if j else NO, 0), (CLIP, 2 * j, j))] + [(CLIP, 12, 7)],
}
WIDE = "blend(add(c0,c1),blend(c2,add(c3,c4)),c5)"
ROT_DEVIATION = {"blend(blend(c0,c1),c2)": 2.72, "add(blend(c0,c1),c2)": 1726.43, WIDE: 246.77, "chain of 8": 2036933.23}  # x 2^-24, measured (see above)
ROT_BOUND = {name: 4 * dev * E for name, dev in ROT_DEVIATION.items()}
SEEDS = {  # per case: the first seed whose scene keeps every slerp decidable, in the float64 and in the float32 run
    ("blend(blend(c0,c1),c2)", "players of 3"): 1, ("blend(blend(c0,c1),c2)", "two graphs"): 2, ("add(blend(c0,c1),c2)", "players of 3"): 1,
    ("add(blend(c0,c1),c2)", "two graphs"): 3, (WIDE, "players of 3"): 1, (WIDE, "two graphs"): 1, ("chain of 8", "players of 3"): 2, ("chain of 8", "two graphs"): 2,
    "a mask on a clip": 1, "a mask on an inner node, inherited by a grandchild": 1, "an inner node of weight 0": 1, "an inner node of weight -1": 1,
    "an inner node of weight NaN": 1, "every child of the root absent": 1}


def slerp(a, v, u, dt):
    dot = (a[0] * v[0] + a[2] * v[2]) + (a[1] * v[1] + a[3] * v[3])
    assert abs(dot) > 1e-3 and abs(abs(dot) - 0.9995) > 1e-4, dot  # the slerp's branches are decidable
    if dot < 0:
        v, dot = -v, -dot
    if dot > dt(0.9995):
        q = a + (v - a) * u
        return q / np.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    th = np.arccos(dot)
    return (a * np.sin(th * (1 - u)) + v * np.sin(th * u)) * (1 / np.sin(th))


def mul(a, b):
    return np.array([((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1], ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0],
                     ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3], ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]])


def evaluate(nodes, masks, k, st, tv, c, groups, rot_bound, dt, eff=0):
    """Component c of one target: node k of `nodes` under the states st -> (value, bound), or None = absent"""
    kind, _, clip = nodes[k]
    eff |= masks.get(k, 0)
    if not st["weight"][k] > 0 or eff & groups:
        return None
    if kind == CLIP:
        return None if tv[clip][c] is None else sample(tv[clip][c][0], tv[clip][c][1], c == 1, tv[clip][c][2], st["seek_time"][k], dt)
    acc = None
    for j in [j for j, nd in enumerate(nodes) if nd[1] == k]:
        r = evaluate(nodes, masks, j, st, tv, c, groups, rot_bound, dt, eff)
        if r is None:
            continue
        (v, b), w = r, dt(st["weight"][j])
        if acc is None:
            acc, bound, wsum = v, b, w
        elif c == 1:
            wsum = wsum + w
            acc, bound = slerp(acc, v, w / wsum, dt) if kind == BLEND else mul(slerp(np.array([0, 0, 0, 1], dt), v, w, dt), acc), rot_bound
        elif kind == BLEND:
            wsum = wsum + w
            acc, bound = acc + (v - acc) * (w / wsum), bound + b + 8 * E * (abs(acc) + abs(v))
        else:
            acc, bound = acc + v * w, bound + abs(w) * b + 4 * E * (abs(acc) + abs(v * w))
    return None if acc is None else (acc, bound)


def graph_scene(seed, sizes, graphs, player_graph, masks=None, idle=()):
    """blend's scene() with sizes[p] targets for player p, who runs graphs[player_graph[p]] (node tables) under node weights 1e-3 .. 1e3
    and seek times of its own; masks: {(graph, node): own mask}; idle: players left alone.  Target i's groups: bit i % 3, and bit 40 if i is odd."""
    sc, rng = scene(seed, [(n, 0) for n in sizes]), np.random.default_rng(seed + 1)
    states, first = [], []
    for p, g in enumerate(player_graph):
        st = np.zeros(len(graphs[g]), B.ANIM_NODE_STATE_DTYPE)
        st["weight"], st["seek_time"] = 10.0 ** rng.uniform(-3, 3, len(st)), rng.uniform(0.2, 0.8, len(st))
        st["weight"][:1], st["weight"][1:][-1:], st["seek_time"][-1] = 1e-3, 1e3, 0.5
        first.append(NO if p in idle else sum(map(len, states)))
        states.append(st)
    i = np.arange(len(sc["targets"]), dtype=np.uint64)
    sc.update(graphs=graphs, player_graph=np.array(player_graph, U32), masks=masks or {}, first_state=np.array(first, U32), states=np.concatenate(states),
              groups=(np.uint64(1) << i % np.uint64(3)) | (i % np.uint64(2) << np.uint64(40)), rot_bound=[0.0] * len(graphs))
    sc["written"] = np.sort(sc["targets"]["row"][sc["first_state"][sc["targets"]["player"]] != NO])
    return sc


def named(seed, sizes, names, player_graph, **kw):
    sc = graph_scene(seed, sizes, [SHAPES[n] for n in names], player_graph, **kw)
    sc["names"], sc["rot_bound"] = names, [ROT_BOUND[n] for n in names]
    return sc


def expected(sc, dt=F64, rot_bound=None):
    want, bound = [c.astype(dt) for c in sc["cur"]], [np.zeros(c.shape) for c in sc["cur"]]
    for tg, tv, groups in zip(sc["targets"], sc["per"], sc["groups"]):
        g, first = sc["player_graph"][tg["player"]], sc["first_state"][tg["player"]]
        if first == NO:
            continue
        masks = {k: m for (gg, k), m in sc["masks"].items() if gg == g}
        for c in range(3):
            r = evaluate(sc["graphs"][g], masks, 0, sc["states"][first:first + len(sc["graphs"][g])], tv, c, int(groups), sc["rot_bound"][g] if rot_bound is None else rot_bound, dt)
            if r is not None:
                want[c][tg["row"]], bound[c][tg["row"]] = r
    return want, bound


def graph_arrays(sc):
    nodes = [(kind, parent, clip, sc["masks"].get((g, k), 0) & 0xFFFFFFFF, sc["masks"].get((g, k), 0) >> 32) for g, gr in enumerate(sc["graphs"]) for k, (kind, parent, clip) in enumerate(gr)]
    sizes = [len(gr) for gr in sc["graphs"]]
    return np.array(list(zip(np.cumsum([0] + sizes[:-1]), sizes)), B.ANIM_GRAPH_DTYPE), np.array(nodes, B.ANIM_GRAPH_NODE_DTYPE)


def graph_targets(sc):
    tg = np.zeros(len(sc["targets"]), B.ANIM_GRAPH_TARGET_DTYPE)
    for f in sc["targets"].dtype.names:
        tg[f] = sc["targets"][f]
    tg["groups_lo"], tg["groups_hi"] = sc["groups"] & np.uint64(0xFFFFFFFF), sc["groups"] >> np.uint64(32)
    return tg


def load(ctx, sc, upload=True):
    start(ctx, sc, upload=False)
    if upload:
        ctx.anim_upload_tracks(sc["tracks"], sc["times"], sc["values"])
        ctx.anim_upload_graphs(*graph_arrays(sc))
        ctx.anim_upload_graph_targets(graph_targets(sc), sc["bindings"], sc["player_graph"])


def changed_rows(ctx):
    ctx.propagate(0)
    return ctx.download_changed_global_transforms()[0]


@pytest.mark.parametrize("k", [0, 1, 2, 5])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_a_flat_graph_is_its_sibling_call_bit_for_bit(n, k):
    """A root BLEND over k clips against anim_frame_blended with the same layers; k = 0: a root CLIP against anim_frame."""
    sc = scene(1000 * n + k, [(n, max(k, 1)), (3, 1)])
    graphs = [([(BLEND, NO, 0)] if k else []) + [(CLIP, 0 if k else NO, clip) for clip, _, _ in kept] for kept in sc["kept"]]
    states = [([(1.0, 0.0)] if k else []) + [(wt, x) for _, x, wt in kept] for kept in sc["kept"]]  # per player: (weight, seek time) of the root, of its clips
    first, states = [0, len(states[0])], states[0] + states[1]
    sc.update(graphs=graphs, masks={}, player_graph=np.array([0, 1], U32), groups=np.zeros(n + 3, np.uint64))
    with B.Context() as a, B.Context() as b:
        start(a, sc), load(b, sc)
        if k:
            a.anim_frame_blended(2, sc["layers"])
        else:
            clip = np.array([sc["kept"][p][0][0] for p in sc["targets"]["player"]])
            a.anim_upload_targets(targets_of(sc["targets"]["row"], sc["targets"]["player"], *[sc["bindings"][CLIPS * np.arange(n + 3) + clip][f] for f in ("track_t", "track_r", "track_s")]))
            a.anim_frame(sc["layers"]["seek_time"])
        b.anim_frame_graph(first, np.array(states, B.ANIM_NODE_STATE_DTYPE))
        got = read_columns(b)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(a), got)) and not np.array_equal(got[1], sc["cur"][1])
        assert np.array_equal(changed_rows(a), changed_rows(b))


NESTED = [(name, layout) for name in SHAPES for layout in ("players of 3", "two graphs")]


def nested_scene(name, layout):
    """65 targets in players of 3 (waves straddle players), or 70 + 30 targets of two graphs (the seam inside what would be one block)"""
    names = list(SHAPES)
    if layout == "players of 3":
        return named(SEEDS[name, layout], [3] * 21 + [2], [name], [0] * 22)
    return named(SEEDS[name, layout], [70, 30], [name, names[(names.index(name) + 1) % 4]], [0, 1])


@pytest.mark.parametrize("name,layout", NESTED)
def test_nested_graphs_against_float64(name, layout):
    sc = nested_scene(name, layout)
    want, bound = expected(sc)
    assert (bound[1] == ROT_BOUND[name]).any()
    with B.Context() as ctx:
        load(ctx, sc)
        ctx.anim_frame_graph(sc["first_state"], sc["states"])
        compare(read_columns(ctx), want, bound, f"{name}, {layout}")
        assert np.array_equal(changed_rows(ctx), sc["written"])


MASKS = {  # on WIDE: (masks, weights set) -- target groups: bit i % 3, bit 40 for odd i
    "a mask on a clip": ({(0, 9): 1 << 0}, {}),
    "a mask on an inner node, inherited by a grandchild": ({(0, 4): 1 << 1, (0, 7): 1 << 40}, {}),
    "an inner node of weight 0": ({}, {4: 0.0}),
    "an inner node of weight -1": ({}, {4: -1.0}),
    "an inner node of weight NaN": ({}, {6: np.nan}),
    "every child of the root absent": ({(0, 9): 1 << 40 | 7}, {1: 0.0, 5: np.nan, 6: -2.0}),
}


def mask_scene(what):
    """Players 0 and 1 (40 and 30 targets) run WIDE, player 2 (5 targets) is left alone"""
    masks, weights = MASKS[what]
    sc = named(SEEDS[what], [40, 30, 5], [WIDE], [0, 0, 0], masks=masks, idle=(2,))
    for node, w in weights.items():
        sc["states"]["weight"][[node, len(SHAPES[WIDE]) + node]] = w
    return sc


@pytest.mark.parametrize("what", list(MASKS))
def test_masks_and_dead_subtrees(what):
    sc = mask_scene(what)
    want, bound = expected(sc)
    if what == "every child of the root absent":
        assert not any(b.any() for b in bound) and all(np.array_equal(w, c) for w, c in zip(want, sc["cur"]))  # nothing is written: bit for bit
    with B.Context() as ctx:
        load(ctx, sc)
        ctx.anim_frame_graph(sc["first_state"], sc["states"])
        compare(read_columns(ctx), want, bound, what)
        assert np.array_equal(changed_rows(ctx), sc["written"]) and len(sc["written"]) == 70  # stamped all the same; the idle player's rows are not


def test_state_equals_an_indexed_upload():
    """Graph frame, then propagate, against an indexed upload of the Transforms it produced on a twin context, then propagate."""
    sc = nested_scene(WIDE, "two graphs")
    n = sc["n"]
    parent = np.full(n, B.NO_PARENT, U32)  # level 0: rows [0, 100), twenty of them with children; level 1: [100, n)
    parent[100:] = np.arange(n - 100) // 2 * 5
    frusta = view_frustum()
    with B.Context() as a, B.Context() as b:
        for ctx in (a, b):
            load(ctx, sc, upload=ctx is a)
            ctx.upload_bounds(np.zeros(3 * n, F32), np.full(3 * n, 0.5, F32))
            ctx.upload_hierarchy(parent, [0, 100, n])
            ctx.propagate_and_cull(frusta, flags=WHOLE)
        a.anim_frame_graph(sc["first_state"], sc["states"])
        cols = read_columns(a)
        b.upload_transforms_indexed(sc["written"], *[c[sc["written"]].reshape(-1) for c in cols])
        for ctx in (a, b):
            ctx.propagate_and_cull(frusta, flags=WHOLE | B.CULL_CHANGED_ROWS)
        (ga, ca), (gb, cb) = a.download_global_transforms(), b.download_global_transforms()
        assert ga.tobytes() == gb.tobytes() and np.array_equal(ca, cb) and np.array_equal(a.download_visibility(0), b.download_visibility(0))
        assert np.array_equal(a.download_changed_global_transforms()[0], b.download_changed_global_transforms()[0])


def frame(ctx, sc, first_state=None):
    ctx.anim_frame_graph(sc["first_state"] if first_state is None else first_state, sc["states"])


def graphs_with(ctx, sc, field, at, value, of="nodes"):
    gr, nd = graph_arrays(sc)
    (nd if of == "nodes" else gr)[field][at] = value
    ctx.anim_upload_graphs(gr, nd)


def targets_with(ctx, sc, player_graph=None, **changes):
    tg, bd = graph_targets(sc), sc["bindings"].copy()
    for field, (at, value) in changes.items():
        (tg if field in tg.dtype.names else bd)[field][at] = value
    ctx.anim_upload_graph_targets(tg, bd, sc["player_graph"] if player_graph is None else player_graph)


INVALID, NOT_READY = api.MI_ERR_INVALID_ARG, api.MI_ERR_NOT_READY
BAD = {  # name -> (the refused call, its error); the scene: player 0 (5 targets) runs add(blend(c0,c1),c2) = nodes 0 .. 4, player 1 (4 targets) WIDE = nodes 5 .. 14
    "an unknown kind": (lambda ctx, sc: graphs_with(ctx, sc, "kind", 0, 3), INVALID),
    "a clip node that is a parent": (lambda ctx, sc: graphs_with(ctx, sc, "kind", 1, CLIP), INVALID),
    "a node range outside the array": (lambda ctx, sc: graphs_with(ctx, sc, "first_node", 1, 6, of="graphs"), INVALID),
    "a graph without nodes": (lambda ctx, sc: graphs_with(ctx, sc, "n_nodes", 0, 0, of="graphs"), INVALID),
    "a graph of 65 nodes": (lambda ctx, sc: ctx.anim_upload_graphs([(0, 65)], [(BLEND, NO, 0, 0, 0)] + [(CLIP, 0, 0, 0, 0)] * 64), INVALID),
    "depth 9": (lambda ctx, sc: ctx.anim_upload_graphs([(0, 9)], [(BLEND, k - 1 if k else NO, 0, 0, 0) for k in range(9)]), INVALID),
    "a parent not below its node": (lambda ctx, sc: graphs_with(ctx, sc, "parent", 2, 2), INVALID),
    "a second root": (lambda ctx, sc: graphs_with(ctx, sc, "parent", 4, NO), INVALID),
    "a target's player >= n_players": (lambda ctx, sc: targets_with(ctx, sc, player=(0, 2)), INVALID),
    "a graph that does not exist": (lambda ctx, sc: targets_with(ctx, sc, player_graph=[0, 2]), INVALID),
    "targets of a player without a graph": (lambda ctx, sc: targets_with(ctx, sc, player_graph=[0, NO]), INVALID),
    "a clip node's clip >= n_clips": (lambda ctx, sc: targets_with(ctx, sc, n_clips=(0, 2)), INVALID),
    "duplicate rows": (lambda ctx, sc: targets_with(ctx, sc, row=(1, sc["targets"]["row"][0])), INVALID),
    "a binding range past the array": (lambda ctx, sc: targets_with(ctx, sc, first_binding=(3, len(sc["bindings"]) - CLIPS + 1)), INVALID),
    "a rotation track in track_t": (lambda ctx, sc: targets_with(ctx, sc, track_t=(0, sc["bindings"]["track_r"][1])), INVALID),
    "states past the array": (lambda ctx, sc: frame(ctx, sc, [0, 6]), INVALID),
    "states for a player without a graph": (lambda ctx, sc: frame(ctx, sc, [0, 5, 0]), INVALID),
    "fewer players than the targets name": (lambda ctx, sc: frame(ctx, sc, [0]), INVALID),
    "a frame before the uploads": (None, NOT_READY),
    "a frame after the tracks dropped the targets": (lambda ctx, sc: (ctx.anim_upload_tracks(sc["tracks"], sc["times"], sc["values"]), frame(ctx, sc)), NOT_READY),
    "a frame after the graphs dropped the targets": (lambda ctx, sc: (ctx.anim_upload_graphs(*graph_arrays(sc)), frame(ctx, sc)), NOT_READY),
}


@functools.lru_cache(None)
def good_frame():
    sc = named(3, [5, 4], ["add(blend(c0,c1),c2)", WIDE], [0, 1])
    with B.Context() as ctx:
        load(ctx, sc)
        frame(ctx, sc)
        return sc, read_columns(ctx)


@pytest.mark.parametrize("what", list(BAD))
def test_argument_checks(what):
    (sc, good), (call, code) = good_frame(), BAD[what]
    with B.Context() as ctx:
        load(ctx, sc, upload=call is not None)
        with pytest.raises(B.MiError) as e:
            (call or frame)(ctx, sc)
        assert e.value.code == code
        if code == NOT_READY:  # (the uploads are made now where there were none, or none any more)
            load(ctx, sc)
        frame(ctx, sc)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(read_columns(ctx), good))
