// kernels_anim.hip -- animation clips in front of the propagate: the Transform animate_targets writes for every animation target of
// a player that plays one clip at weight 1, sampled from a resident pool of keyframe tracks at the player's seek time (kernels.h,
// AnimArgs; the arithmetic is stated in include/bevy_mi355x.h).  ONE launch, a lane per target, 256 targets per workgroup.
//
//   order     mi_anim_upload_targets sorts the targets by player, then by row: the lanes of a wave read one seek time (a wave that
//             straddles two players reads two) and write consecutive rows of the three columns when a rig's joints are.
//   times     the key times the tracks of a workgroup's 256 targets use lie in one range of the pool, found on the host; when it is
//             at most ANIM_LDS_TIMES floats the workgroup copies it into LDS (8 KB, 256 lanes, as many rounds as it takes) and every
//             search and every T[i] / T[i + 1] below reads LDS.  Longer ranges are read where they are: the pool of a clip is a
//             few KB that every wave of the launch shares, so those reads are served by L2.
//   interval  per component, when every lane of the wave that has a track reads the same times -- the same first_time, n_keys and
//             seek time, one wave-uniform compare -- the interval is found ONCE for the wave: the 64 lanes probe 64 evenly spaced
//             keys of the range, a ballot counts the ones <= x and the range shrinks to one stride, until it is 64 keys or fewer
//             (one round for up to 64 keys, two up to 4096).  Otherwise each lane runs its own binary search.
//   values    the keys i and i + 1 of a lane's track come as whole three- or four-float loads (and the two tangents of a
//             CUBIC track); a component without a track is neither read nor written.
//   output    the lane writes its row's translation, rotation (one 16-byte store) and scale, stamps the row's change byte and,
//             when the launch is also the frame's mark_dirty_trees (as k_upload_trs_indexed, kernels_flat.hip), marks the row and
//             its ancestors; the launch zeroes the other half of the marks when asked to.
// Arithmetic: glam_math.h (every operation rounded on its own; -ffp-contract=off); acosf / sinf are the device library's.
// Behind k_anim_frame: k_anim_blend, the same sampling for players that blend several weighted clips (mi_anim_frame_blended), and
// k_anim_graph, for players that run a whole tree of clip, blend and additive nodes with masks (mi_anim_frame_graph).  Last,
// k_anim_weights: the same graphs over weight tracks, n floats per key, into an array of morph weights (mi_anim_frame_weights).
#include "glam_math.h"
#include "kernels.h"

namespace mi {

namespace {

// Where a workgroup reads key times: STAGED, lds[0, n) = pool[lo, lo + n); otherwise the pool itself.  (A template, not a pointer
// chosen at run time: that one is a flat pointer, and every T[j] a flat load.)
template <bool STAGED>
struct AnimTimes {
    const float* pool;
    const float* lds;
    uint32_t lo;
    __device__ __forceinline__ float at(uint32_t j) const {
        if constexpr (STAGED) return lds[j - lo];
        else return pool[j];
    }
};

template <int W>
struct AnimVal {
    float v[W];
};
template <int W>
__device__ __forceinline__ AnimVal<W> anim_load(const float* p) {  // (4-byte aligned: first_value is any float of the pool)
    AnimVal<W> o;
    __builtin_memcpy(&o, p, sizeof o);
    return o;
}

// The largest i with T[i] <= x, for T = times[ft, ft + k) and T[0] < x < T[k - 1], all three wave-uniform; every lane of the wave
// calls it.  Invariant: T[lo] <= x, and the answer lies in [lo, lo + len).
template <bool STAGED>
__device__ __forceinline__ uint32_t anim_wave_interval(const AnimTimes<STAGED>& ts, uint32_t ft, uint32_t k, float x, uint32_t lane) {
    uint32_t lo = 0, len = k;
    while (len > 64u) {
        const uint32_t stride = (len + 63u) >> 6, off = lane * stride;
        const bool le = off < len && ts.at(ft + lo + off) <= x;
        uint32_t c = (uint32_t)__popcll(__ballot(le));  // (the probes ascend: the lanes with T <= x are the first c; lane 0 is one)
        c = c ? c - 1u : 0u;
        lo += c * stride;
        len = len - c * stride < stride ? len - c * stride : stride;
    }
    const bool le = lane < len && ts.at(ft + lo + lane) <= x;
    const uint32_t c = (uint32_t)__popcll(__ballot(le));
    return lo + (c ? c - 1u : 0u);
}
// The same for one lane's own track.
template <bool STAGED>
__device__ __forceinline__ uint32_t anim_lane_interval(const AnimTimes<STAGED>& ts, uint32_t ft, uint32_t k, float x) {
    uint32_t lo = 0, hi = k - 1u;  // T[lo] <= x < T[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ts.at(ft + mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ V4 anim_normalize(V4 q) {
    const float len = f_sqrt(dot4(q, q));
    return V4{f_div(q.x, len), f_div(q.y, len), f_div(q.z, len), f_div(q.w, len)};
}
__device__ __forceinline__ V4 anim_slerp(V4 a, V4 b, float u) {
    float dot = dot4(a, b);
    if (dot < 0.0f) {
        b = V4{-b.x, -b.y, -b.z, -b.w};
        dot = -dot;
    }
    if (dot > 0.9995f) return anim_normalize(a + (b - a) * u);
    const float th = acosf(dot);
    const float sa = sinf(th * (1.0f - u)), sb = sinf(th * u);
    return (a * sa + b * sb) * f_div(1.0f, sinf(th));
}

// One component (W floats; ROT: a quaternion) of one target per lane: out = the lane's track at x; false = the lane has no track.
// Every lane of the wave calls it (live or not): the uniform interval search is the wave's.
template <int W, bool ROT, bool STAGED>
__device__ __forceinline__ bool anim_sample(const AnimArgs& a, const AnimTimes<STAGED>& ts, uint32_t track, bool live, float x, uint32_t lane,
                                            AnimVal<W>& out) {
    const bool has = live && track != ANIM_NO_TRACK;
    const uint64_t has_mask = __ballot(has);
    if (has_mask == 0) return false;
    uint4 d = make_uint4(0u, 1u, 0u, 0u);
    if (has) d = reinterpret_cast<const uint4*>(a.tracks)[track];
    const uint32_t ft = d.x, k = d.y;
    bool first = true, last = false;
    if (has) {
        first = k == 1u || !(x > ts.at(ft));  // (a NaN seek time: the first key)
        if (!first) last = x >= ts.at(ft + k - 1u);
    }
    const bool need = has && !first && !last;  // strictly inside the track: T[0] < x < T[k - 1]
    uint32_t i = last ? k - 1u : 0u;
    if (__ballot(need)) {
        const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(has_mask));
        const uint32_t ft0 = (uint32_t)__builtin_amdgcn_readlane((int)ft, lead), k0 = (uint32_t)__builtin_amdgcn_readlane((int)k, lead);
        const int x0 = __builtin_amdgcn_readlane(__float_as_int(x), lead);
        const bool same = !has || (ft == ft0 && k == k0 && __float_as_int(x) == x0);
        if (__ballot(same) == ~0ull) {  // every lane with a track reads the same times at the same x: one search
            const uint32_t i0 = anim_wave_interval(ts, ft0, k0, __int_as_float(x0), lane);
            if (need) i = i0;
        } else if (need) {
            i = anim_lane_interval(ts, ft, k, x);
        }
    }
    if (!has) return false;
    const uint32_t interp = d.w & ANIM_INTERP_MASK;
    const uint32_t stride = interp == ANIM_CUBIC ? 3u * W : (uint32_t)W, value_at = interp == ANIM_CUBIC ? (uint32_t)W : 0u;
    const float* key = a.values + ((size_t)d.z + (size_t)i * stride);  // key i: [in-tangent,] value [, out-tangent]
    out = anim_load<W>(key + value_at);
    if (!need || interp == ANIM_STEP) return true;
    const float ti = ts.at(ft + i);
    if (x == ti) return true;  // exactly on a key: its value, no interpolation at u = 0
    const float dt = ts.at(ft + i + 1u) - ti;
    const float u = f_div(x - ti, dt);
    const AnimVal<W> va = out, vb = anim_load<W>(key + stride + value_at);
    if (interp == ANIM_LINEAR) {
        if constexpr (ROT) {
            const V4 q = anim_slerp(V4{va.v[0], va.v[1], va.v[2], va.v[3]}, V4{vb.v[0], vb.v[1], vb.v[2], vb.v[3]}, u);
            out.v[0] = q.x, out.v[1] = q.y, out.v[2] = q.z, out.v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) out.v[e] = va.v[e] + (vb.v[e] - va.v[e]) * u;
        }
        return true;
    }
    const AnimVal<W> tan_out = anim_load<W>(key + 2 * W), tan_in = anim_load<W>(key + stride);
    const float u2 = u * u, u3 = u2 * u;
    const float h00 = (2.0f * u3 - 3.0f * u2) + 1.0f, h10 = dt * ((u3 - 2.0f * u2) + u), h01 = 3.0f * u2 - 2.0f * u3, h11 = dt * (u3 - u2);
#pragma unroll
    for (int e = 0; e < W; ++e) out.v[e] = ((h00 * va.v[e] + h10 * tan_out.v[e]) + h01 * vb.v[e]) + h11 * tan_in.v[e];
    if constexpr (ROT) {
        const V4 q = anim_normalize(V4{out.v[0], out.v[1], out.v[2], out.v[3]});
        out.v[0] = q.x, out.v[1] = q.y, out.v[2] = q.z, out.v[3] = q.w;
    }
    return true;
}

// The targets of one workgroup, behind the staging of its key times.
template <bool STAGED>
__device__ __forceinline__ void anim_targets(const AnimArgs& a, const AnimTimes<STAGED>& ts, uint32_t gid) {
    const bool live = gid < a.n_targets;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t row = 0, track_t = ANIM_NO_TRACK, track_r = ANIM_NO_TRACK, track_s = ANIM_NO_TRACK;
    float x = 0.0f;
    if (live) {
        const size_t n = a.n_targets;
        const uint32_t* tg = a.targets + gid;
        row = tg[0];
        x = a.seek[tg[n]];
        track_t = tg[2u * n], track_r = tg[3u * n], track_s = tg[4u * n];
    }
    AnimVal<3> vt, vs;
    AnimVal<4> vr;
    const bool has_t = anim_sample<3, false>(a, ts, track_t, live, x, lane, vt);
    const bool has_r = anim_sample<4, true>(a, ts, track_r, live, x, lane, vr);
    const bool has_s = anim_sample<3, false>(a, ts, track_s, live, x, lane, vs);
    if (!live) return;
    if (has_t) {
        float* o = a.t + 3ull * row;
        o[0] = vt.v[0], o[1] = vt.v[1], o[2] = vt.v[2];
    }
    if (has_r) reinterpret_cast<float4*>(a.r)[row] = make_float4(vr.v[0], vr.v[1], vr.v[2], vr.v[3]);
    if (has_s) {
        float* o = a.s + 3ull * row;
        o[0] = vs.v[0], o[1] = vs.v[1], o[2] = vs.v[2];
    }
    a.changed[row] = (uint8_t)a.changed_gen;  // a stamp, not a flag: see row_changed() in kernels.h
    if (a.mark_bytes) mark_row_and_ancestors(row, a.parent_idx, a.mark_bytes, a.anc, 0xFFFFu);
}

__global__ __launch_bounds__(ANIM_THREADS) void k_anim_frame(AnimArgs a) {
    __shared__ float lds_times[ANIM_LDS_TIMES];
    const uint32_t gid = blockIdx.x * ANIM_THREADS + threadIdx.x;
    if (a.clear_words)
        for (uint32_t w = gid; w < a.n_clear_words; w += gridDim.x * ANIM_THREADS) a.clear_words[w] = 0u;
    if (blockIdx.x >= a.n_target_wgs) return;  // (whole workgroups)
    const uint32_t lo = a.wg_times[2u * blockIdx.x], n = a.wg_times[2u * blockIdx.x + 1u];  // (n <= ANIM_LDS_TIMES: the upload saw to it)
    if (n) {  // (workgroup-uniform)
        for (uint32_t j = threadIdx.x; j < n; j += ANIM_THREADS) lds_times[j] = a.times[lo + j];
        __syncthreads();
        anim_targets<true>(a, AnimTimes<true>{a.times, lds_times, lo}, gid);
    } else {
        anim_targets<false>(a, AnimTimes<false>{a.times, lds_times, 0u}, gid);
    }
}
// ---- blended players (mi_anim_frame_blended; kernels.h, AnimBlendArgs) ---------------------------------------------------------
// 256 threads own 64 consecutive targets; lane j of every wave is target j.  In round r wave w samples layer 4 r + w of its lanes'
// players -- the targets are sorted by player and the four waves differ in the layer, not in the targets, so a wave holds one clip at
// one seek time as a rule and anim_sample finds the key interval once for it -- and leaves ten floats, the weight and a has-mask per
// lane in its quarter of a layer-major LDS tile [4][ANIM_BLEND_COLS][64] (lanes are consecutive words of a column: no bank
// conflicts).  Behind the barrier the fold is split by component: wave 0 folds the translations of the round's four layers in order,
// wave 1 the rotations (the slerp chain), wave 2 the scales, each carrying its accumulator and weight sum in registers across the
// rounds; wave 3 stamps and marks the rows in front of the first round.  The rounds: ceil(most kept layers of the 64 targets / 4), the
// same in every wave without an exchange (all four read the same 64 players).  A second barrier closes a round before the tile is
// written again.  After the last round waves 0 - 2 store one column each.

// One component of the round's four layers folded into (acc, wsum), in layer order: the first contributing layer is taken as it
// is; a later one moves acc by u = weight / (the weights so far + weight).
template <int W, bool ROT>
__device__ __forceinline__ void anim_fold(const float* tile, uint32_t col0, uint32_t bit, uint32_t lane, AnimVal<W>& acc, float& wsum, bool& any) {
#pragma unroll
    for (uint32_t l = 0; l < ANIM_BLEND_WAVES; ++l) {
        const float* c = tile + l * (ANIM_BLEND_COLS * 64u) + lane;
        if (!((__float_as_uint(c[11u * 64u]) >> bit) & 1u)) continue;  // (a wave whose lane has no such layer wrote mask 0)
        AnimVal<W> v;
#pragma unroll
        for (int e = 0; e < W; ++e) v.v[e] = c[(col0 + e) * 64u];
        const float weight = c[10u * 64u];
        if (!any) {
            acc = v, wsum = weight, any = true;
            continue;
        }
        wsum = wsum + weight;
        const float u = f_div(weight, wsum);
        if constexpr (ROT) {
            const V4 q = anim_slerp(V4{acc.v[0], acc.v[1], acc.v[2], acc.v[3]}, V4{v.v[0], v.v[1], v.v[2], v.v[3]}, u);
            acc.v[0] = q.x, acc.v[1] = q.y, acc.v[2] = q.z, acc.v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) acc.v[e] = acc.v[e] + (v.v[e] - acc.v[e]) * u;
        }
    }
}

template <bool STAGED>
__device__ __forceinline__ void anim_blend_targets(const AnimBlendArgs& b, const AnimTimes<STAGED>& ts, float* tile) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t gid = blockIdx.x * ANIM_BLEND_TARGETS + lane;
    uint32_t row = 0, bind0 = 0, stride = 0, first = 0, count = 0;  // count = 0: past the targets, or a player without kept layers
    if (gid < b.n_targets) {
        const size_t n = b.n_targets;
        const uint32_t* tg = b.targets + gid;
        const uint32_t pw = b.players[tg[n]];
        row = tg[0], bind0 = tg[2u * n], stride = tg[3u * n];
        first = pw & ((1u << ANIM_BLEND_COUNT_SHIFT) - 1u), count = pw >> ANIM_BLEND_COUNT_SHIFT;
    }
    if (wave == 3u && count) {
        b.changed[row] = (uint8_t)b.changed_gen;
        if (b.mark_bytes) mark_row_and_ancestors(row, b.parent_idx, b.mark_bytes, b.anc, 0xFFFFu);
    }
    AnimArgs a{};  // what anim_sample reads of it: the two pools
    a.tracks = b.tracks, a.values = b.values;
    AnimVal<4> acc{};  // waves 0 and 2 use three of the four
    float wsum = 0.0f;
    bool any = false;
    for (uint32_t r = 0; __ballot(count > ANIM_BLEND_WAVES * r) != 0; ++r) {  // (the same trips in all four waves)
        const uint32_t l = ANIM_BLEND_WAVES * r + wave;
        const bool on = l < count;
        uint32_t track_t = ANIM_NO_TRACK, track_r = ANIM_NO_TRACK, track_s = ANIM_NO_TRACK;
        float x = 0.0f, weight = 0.0f;
        if (on) {
            const uint32_t* ly = b.layers + 3ull * (first + l);
            const uint32_t* bd = b.bindings + ((size_t)bind0 + (size_t)(3u * ly[0]) * stride);
            x = __uint_as_float(ly[1]), weight = __uint_as_float(ly[2]);
            track_t = bd[0], track_r = bd[stride], track_s = bd[2u * (size_t)stride];
        }
        AnimVal<3> vt{}, vs{};
        AnimVal<4> vr{};
        const bool has_t = anim_sample<3, false>(a, ts, track_t, on, x, lane, vt);
        const bool has_r = anim_sample<4, true>(a, ts, track_r, on, x, lane, vr);
        const bool has_s = anim_sample<3, false>(a, ts, track_s, on, x, lane, vs);
        float* c = tile + wave * (ANIM_BLEND_COLS * 64u) + lane;
        c[0u * 64u] = vt.v[0], c[1u * 64u] = vt.v[1], c[2u * 64u] = vt.v[2];
        c[3u * 64u] = vr.v[0], c[4u * 64u] = vr.v[1], c[5u * 64u] = vr.v[2], c[6u * 64u] = vr.v[3];
        c[7u * 64u] = vs.v[0], c[8u * 64u] = vs.v[1], c[9u * 64u] = vs.v[2];
        c[10u * 64u] = weight;
        c[11u * 64u] = __uint_as_float((has_t ? 1u : 0u) | (has_r ? 2u : 0u) | (has_s ? 4u : 0u));
        __syncthreads();
        if (wave == 0u) {
            AnimVal<3> v3{{acc.v[0], acc.v[1], acc.v[2]}};
            anim_fold<3, false>(tile, 0u, 0u, lane, v3, wsum, any);
            acc.v[0] = v3.v[0], acc.v[1] = v3.v[1], acc.v[2] = v3.v[2];
        } else if (wave == 1u) {
            anim_fold<4, true>(tile, 3u, 1u, lane, acc, wsum, any);
        } else if (wave == 2u) {
            AnimVal<3> v3{{acc.v[0], acc.v[1], acc.v[2]}};
            anim_fold<3, false>(tile, 7u, 2u, lane, v3, wsum, any);
            acc.v[0] = v3.v[0], acc.v[1] = v3.v[1], acc.v[2] = v3.v[2];
        }
        __syncthreads();
    }
    if (!any) return;  // (wave 3; a lane without a contributing layer: the component is not written)
    if (wave == 1u) {
        reinterpret_cast<float4*>(b.r)[row] = make_float4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    } else {
        float* o = (wave == 0u ? b.t : b.s) + 3ull * row;
        o[0] = acc.v[0], o[1] = acc.v[1], o[2] = acc.v[2];
    }
}

__global__ __launch_bounds__(ANIM_BLEND_TARGETS* ANIM_BLEND_WAVES) void k_anim_blend(AnimBlendArgs b) {
    constexpr uint32_t THREADS = ANIM_BLEND_TARGETS * ANIM_BLEND_WAVES;
    __shared__ float lds_times[ANIM_LDS_TIMES];
    __shared__ float tile[ANIM_BLEND_WAVES * ANIM_BLEND_COLS * 64u];
    if (b.clear_words)
        for (uint32_t w = blockIdx.x * THREADS + threadIdx.x; w < b.n_clear_words; w += gridDim.x * THREADS) b.clear_words[w] = 0u;
    if (blockIdx.x >= b.n_target_wgs) return;  // (whole workgroups)
    const uint32_t lo = b.wg_times[2u * blockIdx.x], n = b.wg_times[2u * blockIdx.x + 1u];  // (n <= ANIM_LDS_TIMES: the upload saw to it)
    if (n) {  // (workgroup-uniform)
        for (uint32_t j = threadIdx.x; j < n; j += THREADS) lds_times[j] = b.times[lo + j];
        __syncthreads();
        anim_blend_targets<true>(b, AnimTimes<true>{b.times, lds_times, lo}, tile);
    } else {
        anim_blend_targets<false>(b, AnimTimes<false>{b.times, lds_times, 0u}, tile);
    }
}
// ---- animation graphs (mi_anim_frame_graph; kernels.h, AnimGraphArgs) -----------------------------------------------------------
// 192 threads own 64 consecutive targets of ONE graph (the upload pads at graph seams); lane j of every wave is target j.  The split
// is by component, not by layer: wave 0 runs the graph's whole program for the translations, wave 1 for the rotations, wave 2 for
// the scales.  They never exchange data, so behind the staging of the key times there is no barrier; wave 2 (scales: the component
// a rig most often has no track for) stamps and marks the rows first.  A fourth wave would have nothing to do but that, so 192.
//   program   the host compiled the tree into ENTER / CLIP / LEAVE instructions (kernels.h).  The program counter, the depth and
//             every LDS address are the same in all lanes: instructions are read at a wave-uniform address and moved to SGPRs.
//   alive     which lanes a node counts for is a bit per depth in one VGPR: the parent's bit, the node's weight > 0 in the lane's
//             player, and the node's effective mask against the lane's groups.  ENTER with no lane alive jumps by its skip
//             offset; CLIP with no lane alive samples nothing.  Otherwise every lane calls anim_sample, the dead ones with
//             live = false: the interval search is the wave's.
//   stack     the accumulator of the innermost open node -- value, weight sum -- lives in registers, and whether a level has a
//             value yet is a bit per depth beside `alive`.  ENTER saves the registers (and the entered node's weight) into the
//             wave's LDS stack [level][column][64], LEAVE takes them back and folds the closed node into them: no register array
//             is indexed by the depth.  W + 2 columns a level, 7 levels: 8 960 B for translations and scales, 10 752 B for
//             rotations, 28 672 B a workgroup beside the 8 KB of key times -- 36 KB, four workgroups a CU, three waves a SIMD.

template <int W, bool ROT>
__device__ __forceinline__ void anim_graph_fold(uint32_t kind, AnimVal<W>& acc, float& wsum, bool& any, const AnimVal<W>& v, float weight, bool has) {
    if (!has) return;
    if (!any) {  // the first present child, of a BLEND or an ADD node: as it is
        acc = v, wsum = weight, any = true;
        return;
    }
    if (kind == ANIM_NODE_ADD) {
        if constexpr (ROT) {
            const V4 a = anim_slerp(V4{0.0f, 0.0f, 0.0f, 1.0f}, V4{v.v[0], v.v[1], v.v[2], v.v[3]}, weight);
            const V4 b = V4{acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
            acc.v[0] = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
            acc.v[1] = ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x;
            acc.v[2] = ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w;
            acc.v[3] = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e) acc.v[e] = acc.v[e] + v.v[e] * weight;
        }
        return;
    }
    wsum = wsum + weight;  // (as anim_fold)
    const float u = f_div(weight, wsum);
    if constexpr (ROT) {
        const V4 q = anim_slerp(V4{acc.v[0], acc.v[1], acc.v[2], acc.v[3]}, V4{v.v[0], v.v[1], v.v[2], v.v[3]}, u);
        acc.v[0] = q.x, acc.v[1] = q.y, acc.v[2] = q.z, acc.v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) acc.v[e] = acc.v[e] + (v.v[e] - acc.v[e]) * u;
    }
}

// One wave: the program of its workgroup's graph for component COMP of its 64 targets.  stack: this wave's part of the LDS.
template <int W, bool ROT, uint32_t COMP, bool STAGED>
__device__ void anim_graph_eval(const AnimGraphArgs& g, const AnimTimes<STAGED>& ts, float* stack) {
    constexpr uint32_t LEVEL = (W + 2u) * 64u;
    const uint32_t lane = threadIdx.x & 63u, gid = blockIdx.x * ANIM_GRAPH_TARGETS + lane;  // (gid < n_targets: padded to whole workgroups)
    const size_t n = g.n_targets;
    const uint32_t* tg = g.targets + gid;
    const uint32_t row = tg[0];
    uint32_t first = ANIM_GRAPH_NO_NODE, bind0 = 0, stride = 0;
    uint64_t groups = 0;
    if (row != ANIM_GRAPH_NO_NODE) {
        first = g.first_state[tg[n]];
        bind0 = tg[2u * n], stride = tg[3u * n];
        groups = (uint64_t)tg[4u * n] | (uint64_t)tg[5u * n] << 32;
    }
    const bool active = first != ANIM_GRAPH_NO_NODE;
    if (COMP == 2u && active) {
        g.changed[row] = (uint8_t)g.changed_gen;
        if (g.mark_bytes) mark_row_and_ancestors(row, g.parent_idx, g.mark_bytes, g.anc, 0xFFFFu);
    }
    if (__ballot(active) == 0) return;
    const uint32_t* wg = g.wg + 4u * blockIdx.x;
    const uint32_t prog0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)wg[2]), prog_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)wg[3]);
    AnimArgs a{};  // what anim_sample reads of it: the two pools
    a.tracks = g.tracks, a.values = g.values;
    AnimVal<W> acc{};
    float wsum = 0.0f;
    uint32_t alive = active ? 1u : 0u, present = 0u;  // bit d: the open node of depth d counts for this lane / has a value (bit 0: the result)
    for (uint32_t pc = 0; pc < prog_n;) {
        const uint4 in = reinterpret_cast<const uint4*>(g.prog)[prog0 + pc];
        const uint32_t head = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.x);
        const uint32_t op = head & 3u, d = (head >> 2) & 15u, into = (head >> 6) & 3u, node = (head >> 8) & 0xFFu;
        if (op == ANIM_OP_LEAVE) {  // the open node of depth d is complete: fold it into the one saved at level d - 1
            const float* c = stack + (d - 1u) * LEVEL + lane;
            AnimVal<W> outer;
#pragma unroll
            for (int e = 0; e < W; ++e) outer.v[e] = c[e * 64];
            float outer_wsum = c[W * 64];
            bool outer_any = (present >> (d - 1u)) & 1u;
            anim_graph_fold<W, ROT>(into, outer, outer_wsum, outer_any, acc, c[(W + 1) * 64], (present >> d) & 1u);
            acc = outer, wsum = outer_wsum;
            present = (present & ~(3u << (d - 1u))) | ((outer_any ? 1u : 0u) << (d - 1u));
            ++pc;
            continue;
        }
        float weight = 0.0f, x = 0.0f;
        if (active) {
            const uint32_t* st = g.states + 2ull * ((uint64_t)first + node);
            weight = __uint_as_float(st[0]), x = __uint_as_float(st[1]);
        }
        const uint64_t mask = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)in.z) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)in.w) << 32;
        const bool on = ((alive >> (d - 1u)) & 1u) && weight > 0.0f && (mask & groups) == 0;  // (a NaN weight: not on)
        if (op == ANIM_OP_ENTER) {
            if (__ballot(on) == 0) {  // the subtree is dead in every lane
                pc += head >> 16;
                continue;
            }
            float* c = stack + (d - 1u) * LEVEL + lane;
#pragma unroll
            for (int e = 0; e < W; ++e) c[e * 64] = acc.v[e];
            c[W * 64] = wsum, c[(W + 1) * 64] = weight;
            alive = (alive & ~(1u << d)) | ((on ? 1u : 0u) << d);
            present &= ~(1u << d);
            ++pc;
            continue;
        }
        if (__ballot(on) != 0) {  // ANIM_OP_CLIP
            const uint32_t clip = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.y);
            uint32_t track = ANIM_NO_TRACK;
            if (on) track = g.bindings[(size_t)bind0 + (size_t)(3u * clip + COMP) * stride];
            AnimVal<W> v{};
            const bool has = anim_sample<W, ROT>(a, ts, track, on, x, lane, v);
            bool any = (present >> (d - 1u)) & 1u;
            anim_graph_fold<W, ROT>(into, acc, wsum, any, v, weight, has);
            present |= (any ? 1u : 0u) << (d - 1u);
        }
        ++pc;
    }
    if (!(present & 1u)) return;  // the root is absent for this component: not written
    if constexpr (ROT) {
        reinterpret_cast<float4*>(g.r)[row] = make_float4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
    } else {
        float* o = (COMP == 0u ? g.t : g.s) + 3ull * row;
        o[0] = acc.v[0], o[1] = acc.v[1], o[2] = acc.v[2];
    }
}

template <bool STAGED>
__device__ __forceinline__ void anim_graph_targets(const AnimGraphArgs& g, const AnimTimes<STAGED>& ts, float* stack) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave == 0u) anim_graph_eval<3, false, 0u>(g, ts, stack);
    else if (wave == 1u) anim_graph_eval<4, true, 1u>(g, ts, stack + ANIM_GRAPH_LEVELS * 5u * 64u);
    else anim_graph_eval<3, false, 2u>(g, ts, stack + ANIM_GRAPH_LEVELS * 11u * 64u);
}

__global__ __launch_bounds__(ANIM_GRAPH_TARGETS* ANIM_GRAPH_WAVES) void k_anim_graph(AnimGraphArgs g) {
    constexpr uint32_t THREADS = ANIM_GRAPH_TARGETS * ANIM_GRAPH_WAVES;
    __shared__ float lds_times[ANIM_LDS_TIMES];
    __shared__ float stack[ANIM_GRAPH_LEVELS * 16u * 64u];  // (5 + 6 + 5 columns a level: t, r, s)
    if (g.clear_words)
        for (uint32_t w = blockIdx.x * THREADS + threadIdx.x; w < g.n_clear_words; w += gridDim.x * THREADS) g.clear_words[w] = 0u;
    if (blockIdx.x >= g.n_target_wgs) return;  // (whole workgroups)
    const uint32_t lo = g.wg[4u * blockIdx.x], n = g.wg[4u * blockIdx.x + 1u];  // (n <= ANIM_LDS_TIMES: the upload saw to it)
    if (n) {  // (workgroup-uniform)
        for (uint32_t j = threadIdx.x; j < n; j += THREADS) lds_times[j] = g.times[lo + j];
        __syncthreads();
        anim_graph_targets<true>(g, AnimTimes<true>{g.times, lds_times, lo}, stack);
    } else {
        anim_graph_targets<false>(g, AnimTimes<false>{g.times, lds_times, 0u}, stack);
    }
}
// ---- morph weights (mi_anim_frame_weights; kernels.h, AnimWeightArgs) -----------------------------------------------------------
// A wave owns one chunk: one morph target and 64 consecutive weights of it, lane j the weight j0 + j.  The lanes of a chunk share
// the track, the player and the graph, so everything but the values is the same in all of them and is moved to SGPRs as it is read:
// the chunk, the instruction, the node's state, the mask test, the track, which case of the sampling applies, u and the Hermite
// coefficients, the weight sums.  Four such waves a workgroup, none knowing of the others: no barrier.
//   program   k_anim_graph's, instruction for instruction.  An ENTER whose node does not count is a branch over its skip offset,
//             so no instruction of a dead subtree is ever reached and k_anim_graph's `alive` bits have nothing left to say; whether
//             a level has a value yet (`present`) is a bit per depth in one SGPR.
//   sampling  one track per CLIP: the first / last / NaN cases are two scalar compares, the interval search is anim_wave_interval
//             on the pool itself (at most two rounds of 64 probes), and then each lane loads its float of key i and of key i + 1
//             (and of the two tangents): consecutive floats, 256 B per wave and load.
//   stack     the accumulator of the innermost open node is one VGPR; ENTER saves it into the wave's LDS stack [level][64] with the
//             level's weight sum and the entered node's weight as two words behind it, LEAVE takes them back and folds.  7 levels
//             x 66 words x 4 waves: 7 392 B a workgroup.

__device__ __forceinline__ uint32_t anim_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float anim_unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// anim_graph_fold for one scalar whose weight, weight sum and presence are the wave's
__device__ __forceinline__ void anim_weight_fold(uint32_t kind, float& acc, float& wsum, bool& any, float v, float weight, bool has) {
    if (!has) return;
    if (!any) {
        acc = v, wsum = weight, any = true;
        return;
    }
    if (kind == ANIM_NODE_ADD) {
        acc = acc + v * weight;
        return;
    }
    wsum = wsum + weight;
    const float u = f_div(weight, wsum);
    acc = acc + (v - acc) * u;
}

// The lane's weight of track `tr` (five wave-uniform words) at x; anim_sample's arithmetic for one float.
__device__ __forceinline__ float anim_weight_sample(const AnimWeightArgs& a, const uint32_t* tr, float x, uint32_t j, bool live, uint32_t lane) {
    const uint32_t ft = anim_uni(tr[0]), k = anim_uni(tr[1]), fv = anim_uni(tr[2]), interp = anim_uni(tr[3]), nw = anim_uni(tr[4]);
    const AnimTimes<false> ts{a.times, nullptr, 0u};
    const bool first = k == 1u || !(x > anim_unif(ts.at(ft)));  // (a NaN seek time: the first key)
    const bool last = !first && x >= anim_unif(ts.at(ft + k - 1u));
    const bool need = !first && !last;  // strictly inside the track
    const uint32_t i = need ? anim_uni(anim_wave_interval(ts, ft, k, x, lane)) : (last ? k - 1u : 0u);
    const uint32_t stride = interp == ANIM_CUBIC ? 3u * nw : nw, value_at = interp == ANIM_CUBIC ? nw : 0u;
    const float* key = a.values + ((size_t)fv + (size_t)i * stride + j);  // the lane's float of key i: [in-tangent,] value [, out-tangent]
    float out = 0.0f;
    if (live) out = key[value_at];
    if (!need || interp == ANIM_STEP) return out;
    const float ti = anim_unif(ts.at(ft + i));
    if (x == ti) return out;  // exactly on a key
    const float dt = anim_unif(ts.at(ft + i + 1u)) - ti;
    const float u = f_div(x - ti, dt);
    const float va = out;
    float vb = 0.0f;
    if (live) vb = key[(size_t)stride + value_at];
    if (interp == ANIM_LINEAR) return va + (vb - va) * u;
    float tan_out = 0.0f, tan_in = 0.0f;
    if (live) tan_out = key[2u * (size_t)nw], tan_in = key[stride];
    const float u2 = u * u, u3 = u2 * u;
    const float h00 = (2.0f * u3 - 3.0f * u2) + 1.0f, h10 = dt * ((u3 - 2.0f * u2) + u), h01 = 3.0f * u2 - 2.0f * u3, h11 = dt * (u3 - u2);
    return ((h00 * va + h10 * tan_out) + h01 * vb) + h11 * tan_in;
}

__global__ __launch_bounds__(ANIM_WEIGHT_LANES* ANIM_WEIGHT_WAVES) void k_anim_weights(AnimWeightArgs a) {
    __shared__ float stacks[ANIM_WEIGHT_WAVES * ANIM_GRAPH_LEVELS * ANIM_WEIGHT_LEVEL];
    const uint32_t wave = anim_uni(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t chunk = blockIdx.x * ANIM_WEIGHT_WAVES + wave;
    if (chunk >= a.n_chunks) return;  // (whole waves)
    const uint4 c0 = reinterpret_cast<const uint4*>(a.chunks)[2u * (size_t)chunk], c1 = reinterpret_cast<const uint4*>(a.chunks)[2u * (size_t)chunk + 1u];
    const uint32_t first = anim_uni(a.first_state[anim_uni(c1.y)]);
    if (first == ANIM_GRAPH_NO_NODE) return;  // the player is left alone
    const uint32_t out0 = anim_uni(c0.x), j = (anim_uni(c0.y) & ~63u) + lane, prog0 = anim_uni(c0.z), prog_n = anim_uni(c0.w), bind0 = anim_uni(c1.x);
    const bool live = lane <= (anim_uni(c0.y) & 63u);
    const uint64_t groups = (uint64_t)anim_uni(c1.z) | (uint64_t)anim_uni(c1.w) << 32;
    float* stack = stacks + wave * (ANIM_GRAPH_LEVELS * ANIM_WEIGHT_LEVEL);
    float acc = 0.0f, wsum = 0.0f;
    uint32_t present = 0u;  // bit d: the open node of depth d has a value (bit 0: the result)
    for (uint32_t pc = 0; pc < prog_n;) {
        const uint4 in = reinterpret_cast<const uint4*>(a.prog)[prog0 + pc];
        const uint32_t head = anim_uni(in.x);
        const uint32_t op = head & 3u, d = (head >> 2) & 15u, into = (head >> 6) & 3u, node = (head >> 8) & 0xFFu;
        if (op == ANIM_OP_LEAVE) {  // the open node of depth d is complete: fold it into the one saved at level d - 1
            const float* c = stack + (d - 1u) * ANIM_WEIGHT_LEVEL;
            float outer = c[lane], outer_wsum = anim_unif(c[ANIM_WEIGHT_LANES]);
            bool outer_any = (present >> (d - 1u)) & 1u;
            anim_weight_fold(into, outer, outer_wsum, outer_any, acc, anim_unif(c[ANIM_WEIGHT_LANES + 1u]), (present >> d) & 1u);
            acc = outer, wsum = outer_wsum;
            present = (present & ~(3u << (d - 1u))) | ((outer_any ? 1u : 0u) << (d - 1u));
            ++pc;
            continue;
        }
        const uint32_t* st = a.states + 2ull * ((uint64_t)first + node);
        const float weight = __uint_as_float(anim_uni(st[0])), x = __uint_as_float(anim_uni(st[1]));
        const uint64_t mask = (uint64_t)anim_uni(in.z) | (uint64_t)anim_uni(in.w) << 32;
        const bool on = weight > 0.0f && (mask & groups) == 0;  // (a NaN weight: not on; the node around it is on, or this one is not reached)
        if (op == ANIM_OP_ENTER) {
            if (!on) {  // the subtree is dead
                pc += head >> 16;
                continue;
            }
            float* c = stack + (d - 1u) * ANIM_WEIGHT_LEVEL;
            c[lane] = acc;
            c[ANIM_WEIGHT_LANES] = wsum, c[ANIM_WEIGHT_LANES + 1u] = weight;  // (every lane the same two words)
            present &= ~(1u << d);
            ++pc;
            continue;
        }
        const uint32_t track = on ? anim_uni(a.bindings[(size_t)bind0 + anim_uni(in.y)]) : ANIM_NO_TRACK;  // ANIM_OP_CLIP
        if (track != ANIM_NO_TRACK) {
            const float v = anim_weight_sample(a, a.tracks + (size_t)ANIM_WEIGHT_TRACK_WORDS * track, x, j, live, lane);
            bool any = (present >> (d - 1u)) & 1u;
            anim_weight_fold(into, acc, wsum, any, v, weight, true);
            present |= (any ? 1u : 0u) << (d - 1u);
        }
        ++pc;
    }
    if ((present & 1u) && live) a.weights[(size_t)out0 + lane] = acc;  // (an absent root: the weights keep what they held)
}
}  // namespace

hipError_t launch_anim_weights(AnimWeightArgs a, hipStream_t stream) {
    if (a.n_chunks == 0) return hipSuccess;
    MI_LAUNCH(k_anim_weights, dim3((a.n_chunks + ANIM_WEIGHT_WAVES - 1u) / ANIM_WEIGHT_WAVES), dim3(ANIM_WEIGHT_LANES * ANIM_WEIGHT_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_anim_graph(AnimGraphArgs a, hipStream_t stream) {
    if (a.n_targets == 0) return hipSuccess;
    a.n_target_wgs = a.n_targets / ANIM_GRAPH_TARGETS;
    uint32_t grid = a.n_target_wgs;
    if (a.clear_words) {  // (as launch_anim_frame)
        const uint32_t cb = (a.n_clear_words + 1023u) / 1024u < 1024u ? (a.n_clear_words + 1023u) / 1024u : 1024u;
        grid = grid > cb ? grid : cb;
    }
    if (!a.mark_bytes) a.anc = nullptr;
    MI_LAUNCH(k_anim_graph, dim3(grid), dim3(ANIM_GRAPH_TARGETS * ANIM_GRAPH_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_anim_blend(AnimBlendArgs a, hipStream_t stream) {
    if (a.n_targets == 0) return hipSuccess;
    a.n_target_wgs = (a.n_targets + ANIM_BLEND_TARGETS - 1u) / ANIM_BLEND_TARGETS;
    uint32_t grid = a.n_target_wgs;
    if (a.clear_words) {  // (as launch_anim_frame)
        const uint32_t cb = (a.n_clear_words + 1023u) / 1024u < 1024u ? (a.n_clear_words + 1023u) / 1024u : 1024u;
        grid = grid > cb ? grid : cb;
    }
    if (!a.mark_bytes) a.anc = nullptr;
    MI_LAUNCH(k_anim_blend, dim3(grid), dim3(ANIM_BLEND_TARGETS * ANIM_BLEND_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_anim_frame(AnimArgs a, hipStream_t stream) {
    if (a.n_targets == 0) return hipSuccess;
    a.n_target_wgs = (a.n_targets + ANIM_THREADS - 1u) / ANIM_THREADS;
    uint32_t grid = a.n_target_wgs;
    if (a.clear_words) {  // enough workgroups for the words to clear (as launch_upload_trs_indexed)
        const uint32_t cb = (a.n_clear_words + 1023u) / 1024u < 1024u ? (a.n_clear_words + 1023u) / 1024u : 1024u;
        grid = grid > cb ? grid : cb;
    }
    if (!a.mark_bytes) a.anc = nullptr;
    MI_LAUNCH(k_anim_frame, dim3(grid), dim3(ANIM_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mi
