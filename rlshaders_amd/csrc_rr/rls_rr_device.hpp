// rls_rr_device.hpp -- the workgroup-level form of vndf_microfacet_pair (csrc/rls_device.hpp), for the companion kernel of
// ggx_rr.hip only.  The frozen units never include this header.
//
// vndf_microfacet_pair packs the lanes of ONE wavefront that need the reference's uniform fallback (uniform_slope,
// src/rlGgx.cpp:18-25) into that wavefront's low lanes and runs the fallback once per wavefront: on the mixed-roughness
// workload 97 % of the wavefronts run it, for 7 requests of 64 lanes on average.  Here the requests of the four wavefronts
// of a workgroup tile go to one queue in LDS and ceil(total / 64) wavefronts run the fallback: one pass for the whole tile
// almost always (a tile of the mixed workload holds 29 requests on average).  uniform_slope is a pure function of the two
// words (rx, ry): the same function on the same arguments, on another wavefront.  No arithmetic is touched.
#pragma once

#include "../csrc/rls_device.hpp"

namespace rlsd {

constexpr int kRrWaves = RLS_BLOCK / 64;          // wavefronts per workgroup
constexpr int kRrQueue = 2 * RLS_BLOCK;           // two requests a lane at the most

// LDS of the workgroup form: 2 x 16 B of counts + 4 KB of queue (results overwrite their requests)
struct RrShared {
    float qx[kRrQueue], qy[kRrQueue];             // rx, ry in; slope.x, slope.y out
    uint32_t count[2][kRrWaves];                  // requests per wavefront; double-buffered on the parity of the tile's round
};

// A workgroup barrier that orders LDS accesses only: the streaming loads and stores in flight stay in flight.
RLS_DEV void rr_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Every wavefront of the workgroup calls this with all 64 lanes active, the same number of times (the caller's tile is full:
// a scalar test).  round: how many tiles this workgroup has walked (the parity picks the count buffer); tile: the tile's
// index in the batch (rotates the wavefront that takes a pass, so the extra work is not always one SIMD's).
//
// Barriers: one when no lane of the tile has a request, three otherwise -- `total` is read from LDS after the first barrier,
// so the four wavefronts take the same side.
// Reuse of the LDS by the workgroup's next tile: the count buffers alternate with `round`: a wavefront that has left this
// tile early (total == 0) writes the other buffer, and by the time it writes this one again (two tiles on) every wavefront
// has passed the next tile's first barrier, after its reads here.  The queue needs no second copy: its first write of the
// next tile comes after that tile's first barrier, which every wavefront reaches after its last read here.
RLS_DEV void vndf_microfacet_pair_wg(RrShared &sh, uint32_t round, uint32_t tile,
                                     const VndfView &w, const Frame &fr, float rx1, float ry1, float rx2, float ry2,
                                     V3 &M1, V3 &M2)
{
    V2 s1, s2;
    const bool n1 = vndf_slope_closed(w, rx1, ry1, s1);
    const bool n2 = vndf_slope_closed(w, rx2, ry2, s2);
    const uint64_t m1 = __builtin_amdgcn_ballot_w64(n1), m2 = __builtin_amdgcn_ballot_w64(n2);
    const uint32_t c1 = (uint32_t)__builtin_popcountll(m1), cw = c1 + (uint32_t)__builtin_popcountll(m2);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *count = sh.count[round & 1u];
    count[wave] = cw;                                                               // every lane the same word: one write
    rr_barrier();                                                                   // 1: the four counts are in LDS
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t v = 0; v < (uint32_t)kRrWaves; ++v) {
        const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)count[v]);
        before += v < wave ? c : 0u;
        total += c;
    }
    if (total != 0u) {
        const uint32_t k1 = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
        const uint32_t k2 = before + c1 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2, 0u));
        if (n1) { sh.qx[k1] = rx1; sh.qy[k1] = ry1; }                               // k1, k2 < total <= kRrQueue
        if (n2) { sh.qx[k2] = rx2; sh.qy[k2] = ry2; }
        rr_barrier();                                                               // 2: the queue holds every request
        // pass p (requests 64 p .. 64 p + 63) is wavefront (p + tile) & 3's; passes touch disjoint entries
        for (uint32_t p = (wave - tile) & 3u; p * 64u < total; p += (uint32_t)kRrWaves) {
            uint32_t all = ~0u;                   // the lane number, formed here: it holds no register across the tile loop
            asm volatile("" : "+s"(all));
            const uint32_t q = p * 64u + __builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
            if (q < total) {
                const V2 u = uniform_slope(sh.qx[q], sh.qy[q]);
                sh.qx[q] = u.x;
                sh.qy[q] = u.y;
            }
        }
        rr_barrier();                                                               // 3: the queue holds every result
        if (n1) { s1.x = sh.qx[k1]; s1.y = sh.qy[k1]; }
        if (n2) { s2.x = sh.qx[k2]; s2.y = sh.qy[k2]; }
    }
    M1 = vndf_from_slope(w, fr, s1);
    M2 = vndf_from_slope(w, fr, s2);
}

} // namespace rlsd
