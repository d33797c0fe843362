// decode/run_subframe.h -- the chunk loop of one subframe per lane: which chunk form runs when,
// the redo on the generic path, and the timing probe.
#pragma once
#include "chunk.h"

namespace zflac {

// Timing probe of the chunk loop: nothing in the product build. The -DZFLAC_PROBE build
// (tools/probe.py, run through tools/gpu.sh probe) sums per wave, after DUMMY_BYTES of the
// dummy buffer, 8 u64 counters of k_walk and then 8 of k_decode: the cycles of the top-up, the
// fast part and the generic part, then the chunks, those with every active lane fast, those of
// them redone, the pair chunks, and those of them redone (zflac_hip_probe in abi.cpp reads them).
#ifdef ZFLAC_PROBE
struct ChunkProbe {
    uint64_t t0, t1, t2;
    uint64_t n[8] = {};
    bool was_fast, was_pair;
    __device__ __forceinline__ void start() {
        was_pair = false;
        t0 = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void after_topup() { t1 = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void pair_chunk(bool pair) { was_pair = pair; }
    __device__ __forceinline__ void after_fast(bool lane_slow) {
        t2 = __builtin_amdgcn_s_memtime();
        was_fast = !__builtin_amdgcn_ballot_w64(lane_slow);
    }
    __device__ __forceinline__ void after_slow(bool redo) {
        const uint64_t t3 = __builtin_amdgcn_s_memtime();
        n[0] += t1 - t0;
        n[1] += t2 - t1;
        n[2] += t3 - t2;
        n[3] += 1;
        n[4] += was_fast ? 1 : 0;
        n[5] += (was_fast && redo) ? 1 : 0;
        n[6] += was_pair ? 1 : 0;
        n[7] += (was_pair && redo) ? 1 : 0;
    }
    __device__ __forceinline__ void finish(void* dummy_base, bool walk) {
        unsigned long long* const out =
            reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(dummy_base) + DUMMY_BYTES) + (walk ? 0 : 8);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) atomicAdd(out + i, (unsigned long long)n[i]);
        }
    }
};
#else
struct ChunkProbe {
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void after_topup() {}
    __device__ __forceinline__ void pair_chunk(bool) {}
    __device__ __forceinline__ void after_fast(bool) {}
    __device__ __forceinline__ void after_slow(bool) {}
    __device__ __forceinline__ void finish(void*, bool) {}
};
#endif

// Decode (WALK = false) or walk (WALK = true) one subframe per lane, chunk by chunk.
// WBR: the staged write-back goes through a buffer resource over `out_bytes` of `out`.
template <int KIND, int M, int LAY, bool WALK, bool MIX = false, bool WBR = false>
__device__ __forceinline__ void run_subframe(LaneCtx& L, Rdr& rd, const FrameCtx& fc, void* out, int nch, int c,
                                    int32_t c1m, uint32_t bs_max, void* dummy_base, uint32_t out_bytes = 0) {
    static_assert(!WBR || (!WALK && staged<KIND, LAY>()), "only the staged write-back has a resource form");
    constexpr int L_ = CHUNK;
    static_assert(L_ % hist_len<M>() == 0 && L_ % 16 == 0, "a chunk holds whole history rings and output groups");
    uint4* const dummy = reinterpret_cast<uint4*>(dummy_base) + dummy_slot();
    Pend pd;
    pd.p = dummy;
    pd.v0 = pd.v1 = make_uint4(0, 0, 0, 0);
    StageOf<LAY> sg;
    sg.mask = 0;
    sg.base = 0;
    sg.q0 = (threadIdx.x >> 6) * STAGE_QUADS;
    // (in VGPRs: as a wave-uniform kernel argument it stayed part of the 16-SGPR tuple of the
    // argument load, which the allocator spilled to VGPR lanes and restored with 16 v_readlane
    // at every chunk start's write-back)
    // (the resource form: address and size stay in VGPRs as well, Stage::store_rsrc)
    if constexpr (WBR) {
        const uint64_t o = reinterpret_cast<uintptr_t>(out);
        sg.rw[0] = (uint32_t)o;
        sg.rw[1] = (uint32_t)(o >> 32);
        sg.rw[2] = out_bytes;
    } else {
        uint64_t outv = reinterpret_cast<uintptr_t>(out);
        asm volatile("" : "+v"(outv));
        sg.out = reinterpret_cast<guint4*>(outv);
    }
    if constexpr (!WALK && staged<KIND, LAY>()) {
#pragma unroll
        for (int t = 0; t < 4; t++)  // frame row_frame(t)'s output, in quads (fc.packed: < 2^32)
            sg.gq[t] = (uint32_t)__shfl((int)(uint32_t)(fc.out_elem / 8u), (int)StageOf<LAY>::row_frame(t)) +
                       (StageOf<LAY>::lane() & (StageOf<LAY>::PIECES - 1u));
        if constexpr (WBR) {
#pragma unroll
            for (int t = 0; t < 4; t++) sg.gq[t] <<= 4;  // Stage::store_rsrc takes bytes
        }
    }
    Pred<KIND, M> pr;
    if constexpr (WALK) {
        pr.clear();
    } else {
        if (L.mode != M_NONE) parse_subframe<KIND, M>(L, rd, pr);
        else pr.clear();
    }
    const bool need_pack = !WALK && LAY != LAY_MULTI;  // packed 16-byte stores need aligned frames
    // the subframe's fixed fast-path conditions folded into one per-lane bound (a chunk is fast
    // only if it ends by it): packable output, safe coefficients. (As separate lane masks they
    // were spilled to VGPR lanes and read back at every chunk.)
    const uint32_t fast_bs = ((!need_pack || fc.packed) && !L.unsafe) ? L.bs : 0u;
    // Nothing in flight on loop entry (once per subframe): otherwise the entry edge, where
    // the staged loads are the youngest memory ops, forces vmcnt(0) at every top-up.
    __builtin_amdgcn_s_waitcnt(0);
    uint32_t pair_cool = 0;  // wave-uniform: chunks left before pairs are tried again
    // Adaptive pair back-off (mono kernels): 8, 16, .., 128 chunks as pair failures repeat.
    // Long residual tails (e.g. C2's k = 4 partitions) put a too-long pair in nearly every
    // 64-lane chunk, and each redo on the generic path costs ~6 fast chunks. The stereo
    // kernels keep a fixed 8: the extra wave-uniform state measured 1-3 % slower there.
    constexpr bool BACKOFF = LAY == LAY_MONO;
    uint32_t pair_fail = 0;  // wave-uniform: pair chunks redone since the last good one
    // The form selectors whose inputs are fixed for longer than a chunk, held as wave-uniform lane
    // counts (s_bcnt1 of the ballot: a 32-bit scalar; a bool made from `ballot != 0` went through
    // v_cndmask and v_readfirstlane whenever it was kept across chunks):
    // * ms_bad (all_ms below): lanes that are not mid/side or, 16-bit, have wasted / justify
    //   shifts. Its inputs are fixed once parse_subframe has returned, so it is taken once, over
    //   the lanes with a subframe. Every later chunk's fast lanes are among them: a zero stays
    //   true, and a stale non-zero (the lane has since finished) only picks the generic
    //   decorrelation, which is correct for every channel assignment.
    // * k_bad (fast lanes outside the pair forms' k range, or escaped) and esc_n (fast lanes
    //   escaped) depend on L.k and L.esc, which change only in read_partition_header (at a chunk
    //   start) and in slow_chunk. sel_stale asks for them to be taken again: set at a chunk start
    //   where some lane read a partition header, and after every chunk that ran slow_chunk. In
    //   between the fast lanes can only become fewer (a chunk with a lane that is active but not
    //   fast runs slow_chunk), so a zero stays true and a non-zero is at worst conservative: one
    //   code per step, or the escape form, which decode any k.
    // (HOLD: the walk and the 16-bit pure kernels up to order 16. In the one-wave kernels (order
    // 32, MIX, the larger 32-bit stereo buckets) the held counts moved 25 VGPRs to spill slots, so
    // every other kernel takes its selectors at every chunk, over the chunk's fast lanes, as before.)
    constexpr bool HOLD = WALK || (KIND == 1 && !MIX && M != 32);
    auto count = [](bool p) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(p)); };
    uint32_t sel_stale = 1, k_bad = 0, esc_n = 0, ms_bad = 0;
    if constexpr (HOLD && FormMsOne::template in_kernel<KIND, LAY, MIX, WALK>()) {
        if constexpr (LAY == LAY_STEREO) ms_bad = count(L.mode != M_NONE && L.chan_code != 10);
        if constexpr (KIND == 1) ms_bad += count(L.mode != M_NONE && (L.wasted != 0 || fc.justify != 0));
    }
    ChunkProbe probe;
    auto chunk = [&](uint32_t base) __attribute__((always_inline)) {
        probe.start();
        // (a staged chunk is always the chunk before: sg.mask is 0 at the first)
        topup_st<KIND, LAY, WALK, WBR>(rd, pd, sg, dummy, base - (uint32_t)L_);
        sg.mask = 0;  // flushed
        probe.after_topup();
        const bool part_hdr =
            L.mode == M_PRED && base < L.bs && base >= (uint32_t)L.order && L.left == 0 && L.parts_left > 0;
        if constexpr (HOLD) sel_stale += count(part_hdr);  // (at most 64 a chunk, and reset below: no wrap)
        if (part_hdr) read_partition_header<KIND>(L, rd);
        if (L.mode != M_NONE && rd.pos() > L.end) set_err(L, rd, E_END_OF_STREAM);
        const bool active = L.mode != M_NONE && base < L.bs;
        // The first chunk is fast too: its warm-up samples are re-emitted from the history.
        uint32_t wu;  // warm-up samples in this chunk
        bool lane_fast;
        if constexpr (MIX) {  // constant / verbatim lanes ride along in the mixed variant
            wu = base == 0 && L.mode == M_PRED ? (uint32_t)L.order : 0u;
            const bool pred_ok = L.mode == M_PRED && L.left + wu >= (uint32_t)L_ && !L.unsafe;
            const bool cv_ok = L.mode == M_CONST || (L.mode == M_VERB && L.cbps <= 32);
            lane_fast = active && base + L_ <= L.bs && (pred_ok || cv_ok) && (!need_pack || fc.packed);
        } else {
            wu = base == 0 ? (uint32_t)L.order : 0u;
            lane_fast = active && base + L_ <= fast_bs && L.mode == M_PRED && L.left + wu >= (uint32_t)L_;
        }
        const bool need_slow = active && !lane_fast;
        bool redo = __builtin_amdgcn_ballot_w64(need_slow) != 0;
        if (!redo) {
            // snapshot of the lane's bit position and predictor history: idle lanes get their
            // position back; a long code anywhere sends the whole wave back to redo the chunk
            const uint32_t k_nb = rd.nb;
            const Pred<KIND, M> k_pr = pr;
            if constexpr (!WALK) {
                // frames whose staged output goes back to memory at the next chunk start;
                // cleared again if the chunk is redone
                sg.mask = (typename StageOf<LAY>::Mask)__builtin_amdgcn_ballot_w64(lane_fast && fc.write);
                sg.base = base;
            }
            bool bad = false;
            bool vbad = false;
            uint32_t ovf = 0;
            // ---- the wave-uniform selectors of the chunk's form (chunk.h), in the order taken ----
            // two Rice codes per bit-window step when every fast lane has 1 <= k <= PAIR_KMAX
            // (a selector's compile-time guard is its form's in_kernel: what chunk_in_form runs)
            constexpr auto has = [](auto form) { return decltype(form)::template in_kernel<KIND, LAY, MIX, WALK>(); };
            constexpr bool PAIRS = has(FormPair{});
            // (decode: k >= 2, for rice_step's residual form; the walk takes k = 1 too)
            bool pairs, escs;
            if constexpr (HOLD) {
                if (sel_stale) {  // (see above)
                    sel_stale = 0;
                    k_bad = count(lane_fast && (L.k < (WALK ? 1u : 2u) || L.k > PAIR_KMAX || L.esc));
                    esc_n = count(lane_fast && L.esc);
                }
                pairs = PAIRS && pair_cool == 0 && base != 0 && k_bad == 0;
                escs = esc_n != 0;
            } else {
                pairs = PAIRS && pair_cool == 0 && base != 0 &&
                        __builtin_amdgcn_ballot_w64(lane_fast && (L.k < (WALK ? 1u : 2u) || L.k > PAIR_KMAX || L.esc)) == 0;
                escs = __builtin_amdgcn_ballot_w64(lane_fast && L.esc) != 0;
            }
            // 31/32-bit stereo with decorrelation: the per-sample overflow-checking variant (the
            // generic one-code form, escapes and warm-up included, with the checks), see fast_chunk
            bool wide = false;
            if constexpr (has(FormWide{}))
                wide = __builtin_amdgcn_ballot_w64(lane_fast && L.bps > 30 && L.chan_code >= 8) != 0;
            // constant / verbatim lanes (MIX kernels): one value per step, generic forms
            bool mixed = false;
            if constexpr (has(FormMixed{})) mixed = __builtin_amdgcn_ballot_w64(lane_fast && L.mode != M_PRED) != 0;
            // D_MS: mid/side everywhere (16-bit: and no wasted / justify shifts). Taken only by the
            // ladder's arms below the escapes, like the k >= 2 test of the mono one-code chunks
            // (C2 after its pair back-off).
            auto all_ms = [&]() {
                if constexpr (HOLD) return ms_bad == 0;
                bool ms = true;
                if constexpr (LAY == LAY_STEREO) ms = __builtin_amdgcn_ballot_w64(lane_fast && L.chan_code != 10) == 0;
                if constexpr (KIND == 1)
                    ms = ms && __builtin_amdgcn_ballot_w64(lane_fast && (L.wasted != 0 || fc.justify != 0)) == 0;
                return ms;
            };
            auto mono_res = [&]() {
                return has(FormMonoRes{}) && __builtin_amdgcn_ballot_w64(lane_fast && L.k < 2u) == 0;
            };
            // one chunk in form `form`. `warm_n`: the warm-up samples, for the warm forms (an
            // argument, not the captured `wu`: read through the capture in every form, the MIX
            // kernels came out a few instructions different)
            auto fast = [&](auto form, uint32_t warm_n = 0) {
                chunk_in_form<KIND, M, L_, LAY, MIX, WALK, decltype(form)>(L, rd, pr, base, fc, out, nch, c, c1m, lane_fast,
                                                                           dummy, bad, pd, sg, vbad, ovf, warm_n);
            };
            // `form`, or at a subframe's first chunk its warm-up twin. (Both called from this one
            // lambda, not through `fast`: a lambda inside a lambda changed the MIX kernels' code.)
            auto fast_or_warm = [&](auto form) {
                using Form = decltype(form);
                if (base == 0)
                    chunk_in_form<KIND, M, L_, LAY, MIX, WALK, Warmed<Form>>(L, rd, pr, base, fc, out, nch, c, c1m, lane_fast,
                                                                             dummy, bad, pd, sg, vbad, ovf, wu);
                else
                    chunk_in_form<KIND, M, L_, LAY, MIX, WALK, Form>(L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy,
                                                                     bad, pd, sg, vbad, ovf, wu);
            };
            // ---- the ladder: first match ----
            if (has(FormMixed{}) && mixed) {
                if (wide) fast_or_warm(FormMixedWide{});
                else fast_or_warm(FormMixed{});
            } else if (wide) {
                fast_or_warm(FormWide{});
            } else if (base == 0) {
                fast(FormWarm{}, wu);
            } else if (escs) {
                fast(FormEsc{});
            } else if (!has(FormMsOne{}) || !all_ms()) {
                if (pairs) fast(FormPair{});
                else fast(FormOne{});
            } else if (pairs) {
                fast(FormMsPair{});
            } else if (mono_res()) {
                fast(FormMonoRes{});
            } else {
                fast(FormMsOne{});
            }
            redo = __builtin_amdgcn_ballot_w64(bad && lane_fast) != 0;
            // a pair chunk that had to be redone (codes too long for two per window): one code
            // per step for the next chunks of this subframe (BACKOFF above)
            if (PAIRS && pairs && redo) {
                pair_cool = BACKOFF ? 8u << (pair_fail < 4u ? pair_fail : 4u) : 8u;
                pair_fail++;
            } else if (BACKOFF && PAIRS && pairs) {
                pair_fail = 0;
            } else if (pair_cool) {
                pair_cool--;
            }
            // (wave-uniform: in SGPRs, not a VGPR updated with v_cndmask every chunk)
            pair_cool = __builtin_amdgcn_readfirstlane(pair_cool);
            if constexpr (BACKOFF) pair_fail = __builtin_amdgcn_readfirstlane(pair_fail);
            probe.pair_chunk(PAIRS && pairs && !escs && base != 0);
            if (redo || !lane_fast) {
                rd.nb = k_nb;
            }
            if (redo) {
                pr = k_pr;
                pd.p = dummy;  // the redo rewrites the chunk: drop its pending quads
                sg.mask = 0;   // ... and its staged chunk
            }
            if (!redo && lane_fast) {
                if (!MIX || L.mode == M_PRED) L.left -= L_ - wu;
                L.dom = L.dom || vbad;
                L.dcr |= ovf & (KIND == 1 ? 0x80008000u : 1u);
            }
        }
        probe.after_fast(need_slow);
        if (redo) {
            slow_chunk<KIND, M, L_, LAY, WALK>(L, rd, pr, base, fc, out, nch, c, c1m);
            if constexpr (HOLD) sel_stale = 1;
        }
        probe.after_slow(redo);
    };
    for (uint32_t base = 0; base < bs_max; base += L_) chunk(base);
    probe.finish(dummy_base, WALK);
    if constexpr (!WALK) {
        if constexpr (staged<KIND, LAY>()) {
            sg.template flush<WBR>(dummy, __builtin_amdgcn_readfirstlane(sg.base));
        } else {
            pd.flush(pend_two<KIND>());
        }
    }
    if (L.mode != M_NONE && rd.pos() > L.end) set_err(L, rd, E_END_OF_STREAM);
}

}  // namespace zflac
