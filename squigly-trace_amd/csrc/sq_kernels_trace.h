// sq_kernels_trace.h — the kernels that run with the scene (or the top of its tree) staged in LDS: the persistent trace kernel
// sq_trace_rays / sq_trace_rays_dense and the resident primary pass sq_primary_resident.
#pragma once
#include "sq_frame.h"

// Instruction-arbitration priority of a trace wave (s_setprio) in its return / branch steps, and in its leaf scan and pair windows (and
// the store / refill that follows them).  Priority 1 in the windows, 0 in the steps: with the flat steps the headline frame takes
// 52.4-52.5 ms instead of 53.3-53.4 (levels 1, 2 and 3 alike; raising the STEPS instead costs 0.5 ms), one rank's share at 8 ranks
// 8.09 -> 7.98 ms, the streaming form +-0 (profiles/r03zz5_setprio_flat.txt, r03zz6_setprio_stream.txt).  Round 2 had measured
// -0.5 % for the same setting on the kernels of its time and left it off.
constexpr int kPrioSteps = 0, kPrioWindows = 1;
// Pooled trace kernel: triangles a lane tests per window.  Two in both forms: one owner lookup and one set of pulls serve two tests
// (resident form: 83.0 -> 80.5 ms on the headline frame, same run).
constexpr int kPoolTris = 2;

// The dominant kernel.  Persistent: each wave reserves a chunk of the (dense) ray queue with one
// atomic, compacts the chunk's live entries with ballots into a small LDS list, and each lane pulls
// its next ray from that list as soon as the previous one is finished, so a wave's lanes stay busy
// although ray lengths differ by 10x and although part of the queue is dead.  The first n_lds
// branches (breadth-first = the top of the tree) are staged in LDS once per workgroup; every lane
// keeps its frame stack in LDS (lane-minor layout, one word per frame, at most height-1 frames).
struct TraceArgs {
    float4* org; const float4* dir;          // a finished ray's hit (t bits, triangle) goes into org[slot].xy
    const uint8_t* state; int32_t want;      // a slot is in this launch's queue iff state[slot] == want (kRay1 / kRay2)
    long long front_base; int32_t front;     // front != 0: the queue starts with *n_active extra entries, the slots
                                             //   front_base + [0, *n_active) (the per-pixel mirror rays ride at the head of the
                                             //   first bounce launch instead of having a launch, and a ramp-down, of their own)
    const int32_t* n_active; int32_t k_count; int32_t* head;
    int32_t n_lds; int32_t stack_cap; int32_t straggler_lanes;
    int32_t chunk;               // slots per reservation: a multiple of 64, at most kChunkResident / kChunkStreaming
    int32_t guide_shift;         // towards the end of the queue a reservation shrinks to (slots left >> guide_shift), so that the
                                 //   launch does not end with a few waves still working through a full reservation (first bounce level
                                 //   only by default: on the sparse second-level queue it costs more round trips than it saves, option "guided")
    int32_t refill_min;          // pooled form: idle lanes a wave collects before it fetches new rays for them
    int32_t flush_min;           // pooled form: a trailing part-filled window of the pair pool is run at once from this many pairs on
    int32_t descend_extra, descend_lanes;   // pooled form: further branch steps per iteration for lanes that keep descending, and how many such lanes it takes
    int32_t diag;                // option "coresidency": keep the gauge of live workgroups in stats[24]
    int32_t prio;                // option "trace_prio": s_setprio level of the trace kernel's waves when they start (0 = leave it; the pooled
                                 //   kernel then sets its own levels per phase, kPrioSteps / kPrioWindows, so it only lasts in pool = 0 launches), for the overlapped
                                 //   schedules: per-sample kernels that share a SIMD with a trace workgroup then only get the issue
                                 //   slots the trace waves leave free
    int32_t pixel_major;         // queue ORDER: 0 = slot order (sample-major: neighbouring pixels, one sample each), 1 = all samples
                                 //   of a pixel in a row, so that a wave's rays start from one surface point (slots stay where they are)
    unsigned long long* stats;   // [0] rays traced; PROFILE builds: [1] advance iterations (waves), [2] lanes unwinding,
                                 // [3] lanes descending, [4] leaf iterations (waves), [5] lanes testing a triangle,
                                 // [6] outer iterations (waves), [7] refill executions (waves), [8] lanes refilled
                                 // pooled form: [1] iterations (waves), [2] lanes unwinding, [3] lanes descending,
                                 // [4] pair windows (waves), [5] pairs tested, [6] hits folded, [7] refill executions, [8] lanes refilled,
                                 // [9..13] the return step's TravProf, [14] reserved (reads 0), [16..23] wave time per section of the loop
};
// (the LDS carve-up of the trace kernel, TraceLds and trace_lds_layout: sq_plan.h)

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// Copies the resident form of the scene (sq_scene.h) into the workgroup's LDS and points N / G at it.  The caller syncs.
template <int BLOCK>
__device__ __forceinline__ void stage_resident_scene(const SceneView& S, int n_branches, char* lds, const TraceLds& L, ResidentNodes& N, ResidentTris& G) {
    SQ_LDS v4f* lquads = to_lds<v4f>(lds + L.quads);
    SQ_LDS v2i* lrefs = to_lds<v2i>(lds + L.refs);
    SQ_LDS v4f* lv = to_lds<v4f>(lds + L.verts);
    SQ_LDS v4us* lt = to_lds<v4us>(lds + L.trix);
    for (int i = threadIdx.x; i < n_branches; i += BLOCK) {
        const uint32_t* r = S.rbranch + 10 * (size_t)i;
        lquads[i] = v4f{ __uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3]) };
        lquads[n_branches + i] = v4f{ __uint_as_float(r[4]), __uint_as_float(r[5]), __uint_as_float(r[6]), __uint_as_float(r[7]) };
        lrefs[i] = v2i{ (int)r[8], (int)r[9] };
    }
    // Several loads in flight per thread before the first LDS store (the plain loops wait for every load before the next is issued):
    // a trace launch's staging is on the path of every launch, and a rank's share of a frame at 8 ranks has three launches in 8.5 ms.
    for (int base = threadIdx.x; base < S.n_verts; base += BLOCK * 4) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = base + k * BLOCK; if (i < S.n_verts) v[k] = S.verts4[i]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = base + k * BLOCK; if (i < S.n_verts) lv[i] = v4f{ v[k].x, v[k].y, v[k].z, v[k].w }; }
    }
    for (int base = threadIdx.x; base < S.n_tris; base += BLOCK * 8) {     // vertex indices become byte offsets into the vertex table
        ushort4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int i = base + k * BLOCK; if (i < S.n_tris) t[k] = S.trix[i]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int i = base + k * BLOCK; if (i < S.n_tris) lt[i] = v4us{ (unsigned short)(t[k].x * 16u), (unsigned short)(t[k].y * 16u), (unsigned short)(t[k].z * 16u), t[k].w }; }
    }
    if (threadIdx.x < ResidentTris::kRunPad) lt[S.n_tris + threadIdx.x] = v4us{ 0, 0, 0, 0 };
    N = ResidentNodes{ lquads, lquads + n_branches, lrefs, S.cull_child16 != nullptr, S.cull_child16 };
    G = ResidentTris{ lt };
    if ((uintptr_t)lv != 0) __builtin_trap();                              // the kernels that use this have no static LDS: dynamic LDS starts at address 0
}

// Primary rays with the scene in LDS (the resident form): same per-ray code as sq_primary, but a branch or triangle costs an
// LDS read instead of an L2 round trip.  A primary ray is a chain of ~200 dependent reads, so on small frames -- one rank's
// share of a frame at 8 ranks -- the launch is as long as that chain: 0.58 ms from L2, 0.1-0.2 ms from LDS.
template <typename StackT, int SRC, bool AD, bool SKY, typename FrameT>
__device__ __forceinline__ void primary_resident_body(const SceneView& S, const FrameT& F, const Work& W, int stack_cap, const Sky& K) {
    constexpr bool MV = SRC == kSrcViews;
    extern __shared__ float4 lds_raw[];
    char* lds = reinterpret_cast<char*>(lds_raw);
    const TraceLds L = trace_lds_layout(S.n_branches, true, S.n_verts, S.n_tris, kResidentBlock, stack_cap, (int)sizeof(StackT), false);
    SQ_LDS StackT* stk = to_lds<StackT>(lds + L.stack) + threadIdx.x;
    ResidentNodes N; ResidentTris G;
    stage_resident_scene<kResidentBlock>(S, S.n_branches, lds, L, N, G);
    __syncthreads();
    const long long total = MV ? primary_padded(F) * F.n_views : primary_padded(F);
    for (long long base = (long long)blockIdx.x * kResidentBlock; base < total; base += (long long)gridDim.x * kResidentBlock) {
        int view = 0;
        long long pix;                                                      // (total is a multiple of 64: whole waves)
        if constexpr (SRC == kSrcRays) pix = base + threadIdx.x < (long long)F.h ? base + threadIdx.x : -1;   // index order, as in sq_primary
        else if constexpr (MV) pix = primary_tile_views(F, base + threadIdx.x, view);
        else pix = primary_tile(F, base + threadIdx.x);
        bool in = pix >= 0;
        if constexpr (AD) in = in && pixel_live(F, pix);
        Hit h0; h0.tri = -1; h0.t = 0;
        f3 d0 = sq::mk(0, 0, 0);
        if (in) {
            int y, x;
            if constexpr (SRC == kSrcRays) {
                const f3 o0 = load3(F.ray_org, pix);
                d0 = load3(F.ray_dir, pix);
                h0 = trace_one(S, N, G, S.rroot, o0, d0, stk, kResidentBlock);
            } else if constexpr (MV) {
                pixel_coords(F, pix - (long long)view * F.view_pixels, y, x);
                const ViewCam c = view_cam<true>(F, view);
                d0 = primary_dir(c.rot, F.w, F.h, y, x);
                h0 = trace_one(S, N, G, S.rroot, c.pos, d0, stk, kResidentBlock);
            } else {
                pixel_coords(F, pix, y, x);
                d0 = primary_dir(F.cam_rot, F.w, F.h, y, x);
                h0 = trace_one(S, N, G, S.rroot, sq::mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]), d0, stk, kResidentBlock);
            }
        }
        const int a = wave_append(W.n_active, in && h0.tri >= 0);
        if (a >= 0) store_active<AD>(F, W, a, pix, h0.t, h0.tri);
        else if (in) { if constexpr (SKY) store_miss_sky<AD>(F, pix, K, d0); else store_miss<AD>(F, pix); }
    }
}
template <typename StackT, int SRC, bool AD, typename... SkyT>
__global__ void __launch_bounds__(kResidentBlock) sq_primary_resident(const SceneView S, const FrameOf<SRC> F, const Work W, int stack_cap, const SkyT... K) {
    primary_resident_body<StackT, SRC, AD, sizeof...(SkyT) != 0>(S, F, W, stack_cap, sky_arg<Sky>(K...));
}

template <typename StackT, bool RESIDENT, int BLOCK, bool PROFILE, bool POOL>
__device__ __forceinline__ void trace_rays_body(const SceneView& S, const TraceArgs& A) {
    extern __shared__ float4 lds_raw[];
    char* lds = reinterpret_cast<char*>(lds_raw);
    const TraceLds L = trace_lds_layout(A.n_lds, RESIDENT, S.n_verts, S.n_tris, BLOCK, A.stack_cap, (int)sizeof(StackT), POOL);
    constexpr int kChunk = RESIDENT ? kChunkResident : kChunkStreaming;
    SQ_LDS LiveT* live = to_lds<LiveT>(lds + L.live) + (threadIdx.x >> 6) * kChunk;   // this wave's list
    SQ_LDS StackT* stk = to_lds<StackT>(lds + L.stack) + threadIdx.x;
    SQ_LDS v4f* lquads = to_lds<v4f>(lds + L.quads);
    using NodeSrc = typename std::conditional<RESIDENT, ResidentNodes, HybridNodes>::type;
    using TriSrc = typename std::conditional<RESIDENT, ResidentTris, GlobalTris>::type;
    NodeSrc N; TriSrc G;
    uint32_t root_ref;
    if constexpr (RESIDENT) {                                         // stage the whole scene (coalesced loads)
        stage_resident_scene<BLOCK>(S, A.n_lds, lds, L, N, G);
        root_ref = S.rroot;
    } else {
        for (int i = threadIdx.x; i < 3 * A.n_lds; i += BLOCK) { const float4 q = S.branches[i]; lquads[i] = v4f{ q.x, q.y, q.z, q.w }; }
        N = HybridNodes{ lquads, S.branches_m, (uint32_t)A.n_lds, S.cull_child != nullptr };
        G = GlobalTris{ S.tris, S.leaves, S.packed_leaves != 0, (size_t)S.n_tris * sizeof(DevTri) > ((size_t)4 << 20) };
        root_ref = S.root_ref;
    }
    __syncthreads();
    if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], 1ull);
    if (A.prio == 1) __builtin_amdgcn_s_setprio(1); else if (A.prio == 2) __builtin_amdgcn_s_setprio(2); else if (A.prio == 3) __builtin_amdgcn_s_setprio(3);
    const long long n_front = A.front ? (long long)(*A.n_active) : 0;
    const long long n = (long long)(*A.n_active) * A.k_count + n_front;          // queue positions; slot_of() maps them to slots
    const unsigned n_pix = (unsigned)(*A.n_active), kq = (unsigned)A.k_count;
    auto slot_of = [&](long long q) -> long long {
        if (q < n_front) return A.front_base + q;
        if (!A.pixel_major) return q - n_front;
        const unsigned r = (unsigned)(q - n_front), a = r / kq, k = r - a * kq;   // slot = sample * pixels + pixel (Work)
        return (long long)k * n_pix + a;
    };
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    long long chunk_base = 0;               // wave-uniform
    int my_chunk = A.chunk;                 // wave-uniform: size of this wave's next reservation
    int list_pos = 0, list_len = 0;         // wave-uniform
    bool exhausted = false;                 // wave-uniform
    long long my_ray = -1;
    unsigned long long n_traced = 0;        // wave-uniform
    unsigned long long pf_adv = 0, pf_leaf = 0, pf_outer = 0, pf_refill = 0;   // wave-uniform (PROFILE)
    unsigned int pl_unw = 0, pl_desc = 0, pl_tri = 0, pl_ref = 0;               // per lane (PROFILE)
    Trav T; T.mode = M_DONE; T.sp = 0; T.cur = 0; T.R.tri = -1; T.R.t = 0;
    T.o = T.d = T.df = sq::mk(0, 0, 0);
    int sub_end[3] = { 0, 0, 0 };           // wave-uniform: list positions where the chunk's 2nd, 3rd, 4th 256-slot block start
    auto refill = [&](unsigned long long m, bool idle) {             // m = ballot(idle), wave-uniform
        while (!exhausted && list_pos == list_len) {                    // reserve and compact the next chunk
            int base = 0;
            if (lane == 0) base = atomicAdd(A.head, my_chunk);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= n) { exhausted = true; break; }
            const int this_chunk = my_chunk;
            {   // guided self-scheduling: the next reservation is 1/(4 x waves) of what is left, between 64 and A.chunk slots
                const long long left = n - ((long long)base + this_chunk);
                const long long want = A.guide_shift >= 62 ? (long long)A.chunk : ((left >> A.guide_shift) & ~63ll);
                my_chunk = (int)(want < 64 ? 64 : (want > A.chunk ? A.chunk : want));
            }
            chunk_base = base; list_pos = 0; list_len = 0;
            sub_end[0] = sub_end[1] = sub_end[2] = 0x7fffffff;          // blocks a short reservation does not reach
#pragma unroll
            for (int j = 0; j < kChunk / 64; ++j) {
                if (j * 64 >= this_chunk) break;
                const long long idx = chunk_base + j * 64 + lane;
                const bool alive = idx < n && A.state[slot_of(idx)] == (uint8_t)A.want;
                const unsigned long long am = sq_ballot(alive);
                if (alive) live[list_len + __popcll(am & lt_mask)] = (LiveT)((j & 3) * 64 + lane);   // index within its 256-slot block
                list_len += __popcll(am);
                if ((j & 3) == 3 && j / 4 < 3) sub_end[j / 4] = list_len;
            }
            n_traced += (unsigned long long)list_len;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (exhausted) return;
        const int rank = __popcll(m & lt_mask);
        const int avail = list_len - list_pos;
        if (PROFILE) ++pf_refill;
        if (idle && rank < avail) {
            if (PROFILE) ++pl_ref;
            const int p = list_pos + rank;
            int block = 0;
            if (kChunk > 256) block += p >= sub_end[0];
            if (kChunk > 512) block += p >= sub_end[1];
            if (kChunk > 768) block += p >= sub_end[2];
            my_ray = slot_of(chunk_base + block * 256 + live[p]);
            const float4 o = A.org[my_ray], d = A.dir[my_ray];
            trav_begin(T, S, root_ref, sq::mk(o.x, o.y, o.z), sq::mk(d.x, d.y, d.z));
        }
        list_pos += min(__popcll(m), avail);
    };
    if constexpr (POOL) {
        // Pooled form.  One iteration offers every lane one return (pop a frame), one branch step, and then tests the
        // triangles of ALL leaves the wave's rays have open as a pool of (ray, triangle) pairs: the pairs are numbered
        // by a prefix sum over the lanes' leaf sizes and pair p = 64*window + lane is tested by lane `lane`, whatever
        // ray owns it (the owner's origin, direction and triangle offset come over the DPP/bpermute network).  So a
        // leaf of 14 triangles beside leaves of 3 no longer holds 64 lanes for 14 rounds: the wave runs
        // ceil(sum / 64) full-width rounds.  Accepted hits are folded into the owning lane's R in pair order, which is
        // leaf order, with the very comparison of the one-lane leaf loop (minimumBy's rule, src/BIH.hs:105-109) --
        // the arithmetic of mollerTrumbore does not depend on the lane that runs it.
        constexpr bool kFlat = RESIDENT && !PROFILE;   // the flat steps (sq_scene.h): the resident form only, DESIGN.md 4.8
        bool flat_ok = false;               // wave-uniform (kFlat): every ray of the wave is safe and the scene has culling boxes
        SQ_LDS uint8_t* tab = to_lds<uint8_t>(lds + L.tab) + (threadIdx.x >> 6) * 64;   // this wave's window-head table
        tab[lane] = 0;
        const int lane_tag = lane * 4 + 1;  // a lane's mark in the head table: non-zero, grows with the lane, and is its ds_bpermute address
        int lf_first = 0, lf_cnt = 0;       // M_LEAFQ: the untested rest of this lane's open leaf
        bool carry = false;                 // wave-uniform: the previous iteration left queued pairs untested
        unsigned int pl_hit = 0;
        TravProf prof{};
        // PROFILE: wave time per section of the loop (s_memtime ticks = shader cycles; the stamps themselves cost ~10 %)
        unsigned long long tsec[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, tlast = PROFILE ? __builtin_amdgcn_s_memtime() : 0;
        auto stamp = [&](int sec) { if (PROFILE) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tsec[sec] += now - tlast; tlast = now; } };
        for (;;) {
            if (PROFILE) ++pf_adv;
            const bool idle = (T.mode == M_DONE);
            const unsigned long long m = sq_ballot(idle);       // before the store's exec region: the compare's mask IS the ballot
            if (idle && my_ray >= 0) { *reinterpret_cast<int2*>(A.org + my_ray) = make_int2(__float_as_int(T.R.t), T.R.tri); my_ray = -1; }
            if (m) {
                if (__popcll(m) >= A.refill_min || m == ~0ull) {
                    refill(m, idle);
                    // the flat steps are for waves whose rays are all safe (a ray's flag only changes here) in scenes with culling boxes
                    if constexpr (kFlat) flat_ok = N.cull_on && sq_ballot(T.mode != M_DONE && !T.safe) == 0;
                }
                if (exhausted && m == ~0ull) break;
            }
            stamp(0);
            __builtin_amdgcn_s_setprio(kPrioSteps);                         // return / branch steps (results unchanged)
            if (PROFILE) pl_unw += (T.mode == M_UNWIND);
            if constexpr (kFlat) {
                // the return step with three exec regions (the step, COMBINE, FAR) instead of six nested ones: DONE, the pop and the
                // kind of the popped frame are decided by selects, the FAR half is trav_unwind_far_flat
                if (T.mode == M_UNWIND) {
                    constexpr uint32_t flag = StackTraits<StackT>::flag;
                    const bool done = T.sp == 0;
                    T.sp -= done ? 0 : 1;
                    const uint32_t e = stk[T.sp * BLOCK];                       // (slot 0, unused, for a ray that is done)
                    const bool is_combine = !done && (e & flag) != 0, is_far = !done && (e & flag) == 0;
                    if (is_combine) trav_unwind_combine<TriSrc, StackT>(T, G, e);
                    if (is_far) trav_unwind_far_flat<NodeSrc, StackT>(T, N, stk, BLOCK, e);
                    T.mode = done ? M_DONE : T.mode;
                }
            } else
            if (T.mode == M_UNWIND) trav_unwind(T, N, G, stk, BLOCK, PROFILE ? &prof : nullptr);
            stamp(1);
            if (PROFILE) pl_desc += (T.mode == M_DESCEND);
            if constexpr (kFlat) {
                if (T.mode == M_DESCEND) { if (flat_ok) trav_descend_flat<NodeSrc, StackT>(T, N, stk, BLOCK); else trav_descend(T, N, stk, BLOCK); }
            } else
            if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
            // With the culling boxes a ray takes four branch steps per leaf it opens: lanes that are still descending take up
            // to `descend_extra` more steps in this iteration (while at least `descend_lanes` of them are), instead of paying a
            // whole iteration -- return step, leaf scan, windows -- per branch step.
            for (int x = 0; x < A.descend_extra; ++x) {
                if (__popcll(sq_ballot(T.mode == M_DESCEND)) < A.descend_lanes) break;
                if (PROFILE) pl_desc += (T.mode == M_DESCEND);
                if constexpr (kFlat) {
                    if (T.mode == M_DESCEND) { if (flat_ok) trav_descend_flat<NodeSrc, StackT>(T, N, stk, BLOCK); else trav_descend(T, N, stk, BLOCK); }
                } else
                if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
            }
            stamp(2);
            __builtin_amdgcn_s_setprio(kPrioWindows);                       // ... leaf scan and pair windows
            if constexpr (kFlat) {                                         // open the leaf (src/BIH.hs:105): Nothing so far -- as selects
                const bool open = T.mode == M_LEAF;                         // (a resident leaf reference decodes without a load)
                const int2 lf = G.leaf(T.cur);
                lf_first = open ? lf.x : lf_first; lf_cnt = open ? lf.y : lf_cnt; T.R.tri = open ? -1 : T.R.tri;
                T.mode = open ? (lf.y > 0 ? M_LEAFQ : M_UNWIND) : T.mode;
            } else
            if (T.mode == M_LEAF) {                                         // open the leaf (src/BIH.hs:105): Nothing so far
                const int2 lf = G.leaf(T.cur);
                lf_first = lf.x; lf_cnt = lf.y; T.R.tri = -1;
                T.mode = lf.y > 0 ? M_LEAFQ : M_UNWIND;
            }
            // NT triangles per lane and window.  The pool is counted in UNITS of NT consecutive triangles of one leaf (the
            // last unit of a leaf may be part-filled), so that one owner lookup and one set of pulls serve NT triangle
            // tests: the pulls are the most expensive part of a window (ds_bpermute, 6 cycles per CU each), and the
            // lookup's integer VALU work comes next.
            constexpr int NT = kPoolTris;
            const int c2 = (T.mode == M_LEAFQ) ? lf_cnt : 0;                // triangles left in this lane's open leaf
            if (sq_ballot(c2 > 0) == 0) continue;
            const int u = (c2 + NT - 1) / NT;                               // units
            const int incl = wave_scan_add(u);
            const int U = __builtin_amdgcn_readlane(incl, 63);
            const int start = incl - u;
            const int tb2 = lf_first - NT * start;                          // first triangle of unit q = NT q + tb2
            const int tri_end = lf_first + c2;                              // one past the leaf's last triangle
            int nwin = U >> 6;
            const int rem = U & 63;
            const bool others = sq_ballot(T.mode == M_UNWIND || T.mode == M_DESCEND) != 0;
            if (rem && (!others || carry || rem >= A.flush_min)) ++nwin;
            stamp(3);
            for (int w = 0; w < nwin; ++w) {
                const int base = w << 6;
                const int h = start - base;
                if (u > 0 && h < 64 && incl > base) tab[h > 0 ? h : 0] = (uint8_t)lane_tag;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                int own = tab[lane];
                tab[lane] = 0;
                own = wave_scan_max(own);
                const int q = base + lane;
                const bool act = q < U;
                int tri0 = NT * q + lane_pull(tb2, own);
                const int end_o = lane_pull(tri_end, own);
                const f3 po = sq::mk(lane_pull(T.o.x, own), lane_pull(T.o.y, own), lane_pull(T.o.z, own));
                const f3 pd = sq::mk(lane_pull(T.d.x, own), lane_pull(T.d.y, own), lane_pull(T.d.z, own));
                if (!act) tri0 = 0;                                         // lanes past the last unit test triangle 0 and drop the answer
                stamp(4);
                f3 v0[NT], e1[NT], e2[NT];
                G.template get_run<NT>(tri0, v0, e1, e2);                   // a part-filled unit tests the records after it and drops the answers
                float tt[NT]; bool hit[NT]; unsigned long long hmk[NT], hm = 0;
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const bool valid = act && (k == 0 || tri0 + k < end_o);
                    hit[k] = moller_trumbore_flat(po, pd, v0[k], e1[k], e2[k], tt[k]) & valid;
                }
                stamp(5);
#pragma unroll
                for (int k = 0; k < NT; ++k) { hmk[k] = sq_ballot(hit[k]); hm |= hmk[k]; if (PROFILE) pl_hit += (int)hit[k]; }
                while (hm) {                                                // accepted hits in leaf order: lane by lane, a lane's triangles in turn
                    const int l = __ffsll((long long)hm) - 1;
                    hm &= hm - 1;
                    const int so = __builtin_amdgcn_readlane(own, l);
                    const int stri = __builtin_amdgcn_readlane(tri0, l);
#pragma unroll
                    for (int k = 0; k < NT; ++k) if ((hmk[k] >> l) & 1ull) {
                        const float st = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tt[k]), l));
                        if (lane_tag == so && (T.R.tri < 0 || dist_gt(T.o, T.d, T.R.t, st, T.safe))) { T.R.t = st; T.R.tri = stri + k; }
                    }
                }
                stamp(6);
            }
            const int done = min(U, nwin << 6);                             // units tested
            if (PROFILE) { pf_leaf += nwin; pf_outer += NT * done; }
            if constexpr (kFlat) {
                const bool fin = u > 0 && incl <= done;                     // the Leaf equation is finished: R is its value
                const int adv = (u > 0 && incl > done && start < done) ? NT * (done - start) : 0;   // whole units come first
                T.mode = fin ? M_UNWIND : T.mode; lf_first += adv; lf_cnt -= adv;
            } else
            if (u > 0) {
                if (incl <= done) T.mode = M_UNWIND;                        // the Leaf equation is finished: R is its value
                else if (start < done) { lf_first += NT * (done - start); lf_cnt -= NT * (done - start); }   // whole units come first
            }
            carry = done < U;
            stamp(7);
        }
        if (lane == 0) atomicAdd(&A.stats[0], n_traced);
        if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], ~0ull);   // -1: the workgroup's first wave is leaving (the others follow within a ray's length)
        if (PROFILE) {
            if (lane == 0) { atomicAdd(&A.stats[1], pf_adv); atomicAdd(&A.stats[4], pf_leaf); atomicAdd(&A.stats[5], pf_outer); atomicAdd(&A.stats[7], pf_refill); }
            atomicAdd(&A.stats[2], (unsigned long long)pl_unw); atomicAdd(&A.stats[3], (unsigned long long)pl_desc);
            atomicAdd(&A.stats[6], (unsigned long long)pl_hit); atomicAdd(&A.stats[8], (unsigned long long)pl_ref);
            atomicAdd(&A.stats[9], (unsigned long long)prof.combine); atomicAdd(&A.stats[10], (unsigned long long)prof.recompute_lanes);
            atomicAdd(&A.stats[11], (unsigned long long)prof.recompute_waves); atomicAdd(&A.stats[12], (unsigned long long)prof.slowcmp_lanes);
            atomicAdd(&A.stats[13], (unsigned long long)prof.slowcmp_waves);
            if (lane == 0) for (int i = 0; i < 8; ++i) atomicAdd(&A.stats[16 + i], tsec[i]);
        }
        return;
    }
    for (;;) {
        if (PROFILE) ++pf_outer;
        const bool idle = (T.mode == M_DONE);
        if (idle && my_ray >= 0) { *reinterpret_cast<int2*>(A.org + my_ray) = make_int2(__float_as_int(T.R.t), T.R.tri); my_ray = -1; }
        const unsigned long long m = sq_ballot(idle);
        if (m) {
            refill(m, idle);
            if (exhausted && m == ~0ull) break;
        }
        // advance until (almost) every lane has a leaf to test or is finished
        for (;;) {
            const bool adv = (T.mode == M_DESCEND) || (T.mode == M_UNWIND);
            const unsigned long long am = sq_ballot(adv);
            if (am == 0) break;
            if (__popcll(am) <= A.straggler_lanes && sq_ballot(T.mode == M_LEAF) != 0) break;
            if (PROFILE) { ++pf_adv; pl_unw += (T.mode == M_UNWIND); }
            if (T.mode == M_UNWIND) trav_unwind(T, N, G, stk, BLOCK);
            if (PROFILE) pl_desc += (T.mode == M_DESCEND);
            if (T.mode == M_DESCEND) trav_descend(T, N, stk, BLOCK);
        }
        if (PROFILE) {
            const int cnt = (T.mode == M_LEAF) ? G.leaf(T.cur).y : 0;
            pl_tri += cnt; pf_leaf += wave_max(cnt);
        }
        if (T.mode == M_LEAF) trav_leaf(T, G);
    }
    if (lane == 0) atomicAdd(&A.stats[0], n_traced);
    if (A.diag && threadIdx.x == 0) atomicAdd(&A.stats[kDiagGauge], ~0ull);
    if (PROFILE) {
        if (lane == 0) { atomicAdd(&A.stats[1], pf_adv); atomicAdd(&A.stats[4], pf_leaf); atomicAdd(&A.stats[6], pf_outer); atomicAdd(&A.stats[7], pf_refill); }
        atomicAdd(&A.stats[2], (unsigned long long)pl_unw); atomicAdd(&A.stats[3], (unsigned long long)pl_desc);
        atomicAdd(&A.stats[5], (unsigned long long)pl_tri); atomicAdd(&A.stats[8], (unsigned long long)pl_ref);
    }
}

template <typename StackT, bool RESIDENT, int BLOCK, bool PROFILE, bool POOL>
__global__ void __launch_bounds__(BLOCK) sq_trace_rays(const SceneView S, const TraceArgs A) {
    trace_rays_body<StackT, RESIDENT, BLOCK, PROFILE, POOL>(S, A);
}
// The streaming pooled kernel once more, compiled for SIX waves per SIMD (at most 80 VGPRs; the plain build takes 86, i.e. four):
// three 512-thread workgroups per CU instead of two when their stacks and a share of the tree's top fit in a third of the LDS.
// The streaming form waits on memory two thirds of its time, and the extra waves are worth more than the handful of spilled
// registers and the smaller LDS node prefix: 25.9 -> 24.5 ms (82k triangles), 30.7 -> 29.4 ms (1M triangles) at 64 spp, same
// call (profiles/r03c_stream_incremental.txt, rows libc16 / libw6c16 with incremental = 0).
template <typename StackT>
__global__ void __launch_bounds__(kTraceBlock, 6) sq_trace_rays_dense(const SceneView S, const TraceArgs A) {
    trace_rays_body<StackT, false, kTraceBlock, false, true>(S, A);
}
