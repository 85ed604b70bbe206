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
}  // namespace

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
