// decode/chunk.h -- one chunk of every lane of a wave: the generic slow_chunk, the Rice steps,
// the walk's chunk, fast_chunk and its named forms.
#pragma once
#include "pcm_stage.h"
#include "subframe.h"

namespace zflac {

// Stereo decorrelation (src/zflac.zig:553-578) for lane channel c, c1m = c ? -1 : 0.
// mid/side: R = M - (S >> 1), L = R + S (= zflac's ((M<<1 | S&1) +- S) >> 1 exactly).
template <int DECOR>
__device__ __forceinline__ int32_t decorrelate(uint32_t code, int32_t c1m, int32_t x0, int32_t x1) {
    if constexpr (DECOR == D_MS) {
        return x0 - (x1 >> 1) + (x1 & ~c1m);
    } else {
        // o = (x0 & m0) - ((x1 >> 1) & mh) + (x1 & mp) - (x1 & mn), masks per (code, channel):
        //   LR: c0 x0, c1 x1;  LS(8): c0 x0, c1 x0 - x1;  RS(9): c0 x0 + x1, c1 x1;
        //   MS(10): c0 x0 - (x1 >> 1) + x1, c1 x0 - (x1 >> 1). Arithmetic, not branches.
        const int32_t is_ls = -(int32_t)(code == 8), is_rs = -(int32_t)(code == 9), is_ms = -(int32_t)(code == 10);
        const int32_t is_lr = ~(is_ls | is_rs | is_ms);
        const int32_t m0 = ~(is_lr & c1m) & ~(is_rs & c1m);
        const int32_t mh = is_ms;
        const int32_t mp = (is_lr & c1m) | is_rs | (is_ms & ~c1m);
        const int32_t mn = is_ls & c1m;
        return (x0 & m0) - ((x1 >> 1) & mh) + (x1 & mp) - (x1 & mn);
    }
}

// Does zflac's stereo decorrelation of (x0, x1) overflow the SampleType for output channel
// c (src/zflac.zig:553-578: left/side and side/right in SampleType, mid/side @intCast)?
template <int KIND>
__device__ __forceinline__ bool decor_overflows(uint32_t code, int c, int32_t x0, int32_t x1) {
    int64_t v;
    if (code == 8) {
        if (!c) return false;
        v = (int64_t)x0 - x1;
    } else if (code == 9) {
        if (c) return false;
        v = (int64_t)x0 + x1;
    } else if (code == 10) {
        const int64_t mid = (int64_t)x0 * 2 + (x1 & 1);
        v = c ? (mid - x1) >> 1 : (mid + x1) >> 1;
    } else {
        return false;
    }
    return !fits_sb<KIND>(v);
}

// ----------------------------------------------------------------------------------
// Chunks. A chunk is L_ samples (a multiple of M and of 8) of every lane.
// ----------------------------------------------------------------------------------
// Generic chunk: every mode, warm-up, partition switches and escapes; scalar stores.
template <int KIND, int M, int L_, int LAY, bool WALK>
__device__ __forceinline__ void slow_chunk(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, uint32_t base, const FrameCtx& fc,
                                  void* out, int nch, int c, int32_t c1m) {
    // Rolled over blocks of HM samples (the history ring's period): the generic path is
    // rare, and unrolling it over the whole chunk made it too big for the instruction cache
    constexpr int HM = hist_len<M>();
#pragma unroll 1
    for (uint32_t blk = 0; blk < (uint32_t)(L_ / HM); blk++) {
    static_for<HM>([&](auto uc) {
        constexpr int u = decltype(uc)::value;  // history slot: (blk * HM + u) % HM == u
        const uint32_t i = base + blk * HM + u;
        const bool act = L.mode != M_NONE && i < L.bs;
        int32_t val = 0;
        if (act) {
            rd.ensure(3);
            if (L.mode == M_CONST) {
                val = L.cval;
            } else if (L.mode == M_VERB) {
                const int64_t v = rd.read_signed_wide((uint32_t)L.cbps);
                if (!fits_sb<KIND>(v)) set_err(L, rd, E_OUT_OF_DOMAIN);  // rd_unencoded @intCast (:459)
                val = wrap_st<KIND>((int64_t)((uint64_t)v << L.wasted));
            } else {
                int32_t s;
                if (i < (uint32_t)L.order) {
                    s = pr.template value<u>();
                } else {
                    if (L.left == 0) {
                        if (L.parts_left == 0) set_err(L, rd, E_OUT_OF_DOMAIN);
                        else read_partition_header<KIND>(L, rd);
                    }
                    const int64_t r = residual_general<KIND>(L, rd);
                    L.left--;
                    if constexpr (WALK) {
                        s = 0;
                    } else {
                        const int64_t p = pr.template predict<u>(L.shift);
                        // exact r + prediction: InterType overflow (:531 `+=`) or a value
                        // outside the SampleType (:494,537 @intCast) is OutOfDomain
                        const int64_t sx = (int64_t)((uint64_t)r + (uint64_t)p);
                        if constexpr (KIND != 2)
                            if (L.unsafe && !pr.template partials_fit<u>(L.order)) L.dom = true;
                        if (!fits_sb<KIND>(sx)) L.dom = true;
                        s = add_inter<KIND>(r, p);
                        pr.template push<u>(s);
                    }
                }
                val = wrap_st<KIND>((int64_t)((uint64_t)(int64_t)s << L.wasted));
            }
        }
        if constexpr (!WALK) {
            int32_t o = val;
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(val, x0, x1);
                o = decorrelate<D_GEN>(L.chan_code, c1m, x0, x1);
                if (act && decor_overflows<KIND>(L.chan_code, c, x0, x1)) L.dcr = 1;
            }
            if (act && fc.write) store_elem<KIND>(out, fc.out_elem + (uint64_t)nch * i + c, o << fc.justify);
        }
    });
    }
}

// v_ffbh_u32 with the hardware's result for 0 (0xFFFFFFFF); __builtin_clz(0) is undefined.
__device__ __forceinline__ uint32_t ffbh_raw(uint32_t x) {
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// Rice codes of one bit-window step (src/zflac.zig:657-663). NC = 1: one code from the
// 32-bit peek, `lim` tracks the smallest peek (a peek below 2^k holds no whole code).
// NC = 2: two codes from the same peek, `lim` tracks the largest bit count of a step (more
// than 32 means the pair did not fit). Needs 1 <= k: with k >= 1 a peek of 0 yields a
// count above 32 through ffbh's 0xFFFFFFFF. Returns the bits consumed.
//
// RES (NC = 2, needs 2 <= k): zz receives the residuals themselves, zigzag included. With
// y = h << (q + 1) (the code's remainder at the top), zz >> 1 = (q << (k-1)) | (rem >> 1) is
// one v_alignbit of (q, y) by 33 - k, and -(zz & 1) one v_bfe_i32 of y at 32 - k: the
// residual is their xor, which the caller's add fuses into a v_xad. (k = 1 would need an
// alignbit by 32, which the hardware reads as 0.)
template <int NC, bool ESC, bool RES = false, bool WALK = false>
__device__ __forceinline__ uint32_t rice_step(uint32_t h, uint32_t k, uint32_t kp1, uint32_t& lim, uint32_t (&zz)[NC],
                                              bool esc, uint32_t escw, int32_t& escv) {
    if constexpr (NC == 1) {
        if constexpr (ESC) {
            // escape partition (src/zflac.zig:646-653): escw-bit signed values, escw = 0 -> zeros
            lim = esc ? lim : min(lim, h);
            const uint32_t q = ffbh_raw(h);
            const uint32_t len = esc ? escw : q + kp1;
            if constexpr (!WALK) {
                zz[0] = (q << k) | __builtin_amdgcn_ubfe(h, 32 - (q + kp1), k);
                escv = escw ? ((int32_t)h >> (32 - escw)) : 0;
            }
            return len;
        } else if constexpr (RES) {  // the residual itself (2 <= k), as in the pair form below
            static_assert(!WALK, "residual values are decode-only");
            lim = min(lim, h);  // a garbage y (q >= 31, h = 0) comes with a flagged peek
            const uint32_t q = ffbh_raw(h);
            const uint32_t y = h << ((q + 1u) & 31u);
            zz[0] = __builtin_amdgcn_alignbit(q, y, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y, 32u - k, 1u);
            return q + kp1;
        } else {
            lim = min(lim, h);
            const uint32_t q = __builtin_clz(h);
            const uint32_t len = q + kp1;
            if constexpr (!WALK) zz[0] = (q << k) | __builtin_amdgcn_ubfe(h, 32 - len, k);
            return len;
        }
    } else if constexpr (RES) {
        static_assert(!WALK, "residual values are decode-only");
        // q >= 31 (or h = 0: q = ~0) makes y garbage, but then tot > 32 flags the step
        const uint32_t q1 = ffbh_raw(h);
        const uint32_t y1 = h << ((q1 + 1u) & 31u);
        const uint32_t g = (y1 << k) | 1u;  // the second code; bit 0 stops ffbh at 31
        const uint32_t q2 = ffbh_raw(g);
        const uint32_t y2 = g << ((q2 + 1u) & 31u);
        const uint32_t tot = q1 + q2 + 2u * kp1;
        lim = max(lim, tot);
        zz[0] = __builtin_amdgcn_alignbit(q1, y1, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y1, 32u - k, 1u);
        zz[1] = __builtin_amdgcn_alignbit(q2, y2, 33u - k) ^ (uint32_t)__builtin_amdgcn_sbfe((int)y2, 32u - k, 1u);
        return tot;
    } else {
        const uint32_t q1 = ffbh_raw(h);
        const uint32_t l1 = q1 + kp1;
        const uint32_t g = (h << l1) | 1u;  // the second code; bit 0 stops ffbh at 31
        const uint32_t q2 = ffbh_raw(g);
        const uint32_t tot = l1 + q2 + kp1;
        lim = max(lim, tot);
        if constexpr (!WALK) {
            zz[0] = (q1 << k) | __builtin_amdgcn_ubfe(h, 32 - l1, k);
            zz[1] = (q2 << k) | __builtin_amdgcn_ubfe(h, 32 - tot, k);
        }
        return tot;
    }
}

// (m & a) | (~m & b) as one v_bfi_b32
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

// The walk's steps (k_walk, lengths only): nothing in a walk step can hide the latency of a
// ring read, so the walk keeps the window in registers: (w0, w1) = ring words an-2 and an-1
// at shift sh, wn = word an, wn1 = word an+1, and each step reads word an+2 for the step
// after it (its address does not depend on the step): step s's read is selected in only at
// the end of step s+1, a whole step after its issue. An advance (the sign of sh - n, as a
// mask) shifts the window by one word with v_bfi_b32 selects (v_cndmask on a borrow in VCC
// needs two wait states after the write, which a walk step has no independent work to fill).
// The ring holds the words byte-swapped. nb is rebuilt from the advances at the end. A step
// moves the window by at most one word: a longer (flagged) step leaves a wrong position,
// which the redo discards.
template <int L_, int NC, bool ESC, bool WARM>
__device__ __forceinline__ void walk_steps(Rdr& rd, uint32_t k, uint32_t kp1, uint32_t& lim, bool esc, uint32_t escw,
                                           uint32_t wu) {
    const uint32_t nb0 = rd.nb;
    const uint32_t t0 = nb0 << 3;  // slot bits of word an-1 (see Rdr); an-2 is one slot up
    uint32_t w1 = rd.lds_word(rd.ldsb() | (t0 & RING_SLOT_MASK));
    uint32_t w0 = rd.lds_word(rd.ldsb() | ((t0 + 256u) & RING_SLOT_MASK));
    uint32_t wn = rd.lds_word(rd.ldsb() | ((t0 - 256u) & RING_SLOT_MASK));
    uint32_t wn1 = rd.lds_word(rd.ldsb() | ((t0 - 512u) & RING_SLOT_MASK));
    uint32_t pa = t0 - 768u;  // slot bits of word an+2: 256 lower per advance
    uint32_t sh = nb0 & 31u;
    uint32_t m_prev = 0, nx_prev = 0;
    static_for<L_ / NC>([&](auto sc) {
        constexpr int u0 = decltype(sc)::value * NC;
        const uint32_t nx = rd.lds_word(rd.ldsb() | (pa & RING_SLOT_MASK));  // word an+2
        uint32_t zz[NC];
        int32_t escv = 0;
        uint32_t n = rice_step<NC, ESC, /*RES=*/false, /*WALK=*/true>(__builtin_amdgcn_alignbit(w0, w1, sh), k, kp1, lim, zz,
                                                                      esc, escw, escv);
        if constexpr (WARM) n = (uint32_t)u0 < wu ? 0u : n;
        const uint32_t tu = sh - n;
        const uint32_t m = (uint32_t)((int32_t)tu >> 31);
        sh = tu & 31u;
        // word an+1 of this step's an (the previous step's read): the empty asm ties the read's
        // first use to this step's position, so its wait comes after this step's own read is
        // issued, a whole step after its own issue (left alone, the scheduler hoists the select
        // into the step that issued the read and waits for it there)
        asm("" : "+v"(nx_prev) : "v"(tu));
        wn1 = bfi(m_prev, nx_prev, wn1);
        w0 = bfi(m, w1, w0);
        w1 = bfi(m, wn, w1);
        wn = bfi(m, wn1, wn);
        // pa -= 256 on an advance: m shifted into place and added in one v_lshl_add_u32
        asm("v_lshl_add_u32 %0, %1, 8, %2" : "=v"(pa) : "v"(m), "v"(pa));
        m_prev = m;
        nx_prev = nx;
    });
    rd.nb = (nb0 & ~31u) - ((t0 - 768u - pa) >> 3) + sh;
}

// ----------------------------------------------------------------------------------
// Chunk forms. A form is what one fast (or walk) chunk is compiled for: the stereo
// decorrelation (D_GEN: any channel assignment and shifts; D_MS: mid/side in every lane, and
// for 16-bit containers no wasted-bits or justify shift), NC Rice codes per bit-window step,
// and the flags below (see fast_chunk). run_subframe picks one form per chunk.
// ----------------------------------------------------------------------------------
enum FormFlag : unsigned {
    F_ESC = 1,     // lanes may be in an escape partition
    F_WARM = 2,    // a subframe's first chunk: its warm-up samples are re-emitted
    F_MIXED = 4,   // lanes may be CONSTANT or VERBATIM subframes (MIX kernels)
    F_RES1 = 8,    // one code per step, taken as the residual itself (every fast lane has k >= 2)
    F_WIDE = 16,   // per-sample decorrelation overflow check (31/32-bit stereo)
};
// The kernels with two codes per step, and those with the mid/side forms (the others decode
// every chunk with the generic decorrelation).
template <int KIND, bool WALK>
__device__ __forceinline__ constexpr bool has_pairs() { return WALK || KIND == 1; }
template <int KIND, int LAY, bool WALK>
__device__ __forceinline__ constexpr bool has_ms() {
    return !(WALK || LAY == LAY_MULTI || KIND == 0 || (KIND == 2 && LAY == LAY_MONO));
}

template <int DECOR_, int NC_, unsigned FLAGS_ = 0>
struct ChunkForm {
    static constexpr int DECOR = DECOR_, NC = NC_;
    static constexpr unsigned FLAGS = FLAGS_;
    static constexpr bool ESC = (FLAGS & F_ESC) != 0, WARM = (FLAGS & F_WARM) != 0, MIXED = (FLAGS & F_MIXED) != 0,
                          RES1 = (FLAGS & F_RES1) != 0, WIDE = (FLAGS & F_WIDE) != 0;
    static_assert(NC == 1 || NC == 2);
    static_assert(!WARM || NC == 1, "warm-up chunks decode one code per step");
    static_assert(!MIXED || (NC == 1 && ESC), "mixed chunks: one value per step");
    static_assert(!RES1 || (NC == 1 && !ESC && !WARM && !MIXED), "RES1: plain one-code decode chunks");
    static_assert(!WIDE || DECOR == D_GEN, "WIDE: the generic decorrelation with its checks");
    // Does kernel (container, layout, MIX; walk or decode) have this form? A kernel instantiates
    // no other: each form is thousands of instructions in the order-32 kernels.
    template <int KIND, int LAY, bool MIX, bool WALK>
    static constexpr bool in_kernel() {
        return (NC == 1 || has_pairs<KIND, WALK>()) && (DECOR == D_GEN || has_ms<KIND, LAY, WALK>()) &&
               (!RES1 || LAY == LAY_MONO) && (!MIXED || (MIX && !WALK)) && (!WIDE || (KIND == 2 && LAY == LAY_STEREO));
    }
};
// The forms launched today, and when run_subframe chooses each (first match, in this order):
using FormMixed = ChunkForm<D_GEN, 1, F_ESC | F_MIXED>;               // a constant / verbatim lane among the fast
using FormMixedWide = ChunkForm<D_GEN, 1, F_ESC | F_MIXED | F_WIDE>;  // ... and a 31/32-bit decorrelated lane
using FormWide = ChunkForm<D_GEN, 1, F_ESC | F_WIDE>;                 // a 31/32-bit decorrelated stereo lane
using FormWarm = ChunkForm<D_GEN, 1, F_ESC | F_WARM>;                 // the subframe's first chunk
using FormEsc = ChunkForm<D_GEN, 1, F_ESC>;                           // a lane in an escape partition
using FormPair = ChunkForm<D_GEN, 2>;          // not all mid/side; pairs: every k in 2 (walk: 1)..PAIR_KMAX
using FormOne = ChunkForm<D_GEN, 1>;           // not all mid/side, no pairs
using FormMsPair = ChunkForm<D_MS, 2>;         // all mid/side (mono: always), pairs
using FormMonoRes = ChunkForm<D_MS, 1, F_RES1>;  // mono, no pairs, every k >= 2
using FormMsOne = ChunkForm<D_MS, 1>;          // all mid/side, else
// The first three at a subframe's first chunk (base == 0): the same with the warm-up samples.
template <typename Form>
using Warmed = ChunkForm<Form::DECOR, Form::NC, Form::FLAGS | F_WARM>;
using FormMixedWarm = Warmed<FormMixed>;
using FormMixedWideWarm = Warmed<FormMixedWide>;
using FormWideWarm = Warmed<FormWide>;

// The walk's chunk (k_walk): the lengths of L_ codes, no samples. `bad` as in fast_chunk.
template <int L_, typename Form>
__device__ __forceinline__ void walk_chunk(LaneCtx& L, Rdr& rd, bool& bad, uint32_t wu) {
    uint32_t lim = Form::NC == 1 ? 0xFFFFFFFFu : 0u;
    walk_steps<L_, Form::NC, Form::ESC, Form::WARM>(rd, L.k, L.kp1, lim, L.esc, L.escw, wu);
    const bool dry = rd.dry();
    if constexpr (Form::NC == 1) bad |= lim < L.thr || dry;
    else bad |= lim > 32u || dry;
}

// Fast chunk: every lane that is `lane_fast` is a predicted subframe with >= L_ Rice codes
// left in its partition, past its warm-up. Straight-line, fully unrolled, no branch: a code
// (or, for NC = 2, a pair of codes) longer than the 32-bit peek only raises `bad` (the
// caller redoes the chunk on the generic path). Lanes that are not fast decode garbage that
// the caller rolls back. 16-bit containers keep samples as the predictor's packed pairs:
// stereo decorrelation, shifts and interleave run once per 8 samples on i16 pairs.
// Value ranges: `vbad` = some sample left the SampleType (or, 32-bit containers, the
// prediction sum left i32); `ovf` = decorrelation overflow bits. The caller keeps both only
// when the chunk is not redone. (Fast lanes are `safe`: no partial LPC sum can overflow and
// |r| <= 2^30, so the 8/16-bit `r + prediction` below is exact in i32.)
// WARM (a subframe's first chunk, NC = 1): samples u < `wu` (= the predictor order) are the
// warm-up samples already in the history; they consume no bits and are only re-emitted.
// MIXED (NC = 1, with ESC): lanes may also be CONSTANT (no bits, the constant) or VERBATIM
// (cbps <= 32 bits per sample, src/zflac.zig:455-465) subframes; a verbatim value outside the
// SampleType sends the chunk back to the generic path (zflac fails at that read).
template <int KIND, int M, int L_, int LAY, typename Form>
__device__ __forceinline__ void fast_chunk(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, uint32_t base, const FrameCtx& fc,
                                           void* out, int nch, int c, int32_t c1m, bool lane_fast, uint4* dummy,
                                           bool& bad, Pend& pd, StageOf<LAY>& sg, bool& vbad, uint32_t& ovf,
                                           uint32_t wu) {
    constexpr int DECOR = Form::DECOR, NC = Form::NC;
    constexpr bool ESC = Form::ESC, WARM = Form::WARM, MIXED = Form::MIXED, WIDE = Form::WIDE;
    // decode pairs take their residuals straight from rice_step (every fast lane has k >= 2)
    // (RES1: one-code chunks of the mono kernels in waves where every fast lane has k >= 2)
    constexpr bool RES = NC == 2 || Form::RES1;
    const bool is_verb = MIXED && L.mode == M_VERB, is_const = MIXED && L.mode == M_CONST;
    // 32-bit containers, stereo: the decorrelation runs in wrapping i32, which is exact
    // whenever zflac's result fits the SampleType; with 31- or 32-bit decorrelated samples
    // in the wave it can also overflow it (src/zflac.zig:558,564 checked, :573-574
    // @intCast), which the WIDE variant checks per sample. (WIDE is a template argument,
    // chosen once per chunk: a per-sample branch would cut the unrolled chunk into one
    // basic block per sample, and the scheduler could no longer overlap one sample's
    // older-history MACs with the previous sample's chain.)
    static_assert(!WIDE || (KIND == 2 && LAY == LAY_STEREO), "WIDE: 31/32-bit stereo only");
    constexpr bool wide = WIDE;
    const uint32_t vshift = 32u - (uint32_t)L.cbps;  // verbatim: top cbps bits of the peek
    bool vrange = false;                            // a verbatim value outside the SampleType
    const uint32_t k = L.k, kp1 = L.kp1;
    const int shift = L.shift;
    const uint32_t wasted = (uint32_t)L.wasted;
    const uint32_t justify = fc.justify;
    const bool do_store = lane_fast && fc.write;
    constexpr bool PACK16 = KIND == 1 && LAY != LAY_MULTI;
    constexpr bool SHIFTS = DECOR != D_MS;  // D_MS is only chosen when no lane shifts
    DecMasks dm;
    if constexpr (DECOR == D_GEN) dm.init(L.chan_code);
    uint32_t pk[KIND == 2 ? 8 : 4];
    uint32_t pb = 0, pb2 = 0;  // 8-bit containers: samples of the dword being packed
    uint32_t lim = NC == 1 ? 0xFFFFFFFFu : 0u;
    int32_t vmax = 0, vmin = 0;  // range of the chunk's samples (8/16-bit containers)
    bool v32 = false;            // 32-bit containers: a sum outside i32
    // 32-bit containers, stereo, not WIDE: bit 31 set once a sample entering the decorrelation
    // lies outside [-2^30, 2^30): a predicted sample may leave the stream's depth (zflac keeps
    // whatever fits the SampleType), and then the wrapping i32 decorrelation below is no longer
    // known to be exact. Such a chunk goes back to the generic path and its per-sample checks.
    uint32_t big = 0;
    // packed output of 8 samples: stored at once, except the chunk's last group, which stays
    // pending until after the next chunk-start wait (a store issued just before that wait
    // would expose its whole latency)
    auto emit = [&](auto last, uint4* p, uint4 v0, uint4 v1) {
        if constexpr (decltype(last)::value) {
            pd.p = p;
            pd.v0 = v0;
            pd.v1 = v1;
        } else {
            p[0] = v0;
            if constexpr (pend_two<KIND>()) p[1] = v1;
        }
    };
    // one sample: residual -> prediction -> history -> packed output every 8 samples
    auto sample = [&](auto uc, int64_t r, bool warm, int32_t vv) {
        constexpr int u = decltype(uc)::value;
        const uint32_t i = base + u;
        const int64_t p = pr.template predict<u>(shift);
        // a warm-up sample re-enters the history as itself (its pair's low half, s[-1] for
        // u = 0, only ever meets a zero coefficient); it was range-checked when read
        int32_t s;
        if constexpr (KIND == 2) {
            int64_t sx = (int64_t)((uint64_t)r + (uint64_t)p);
            if constexpr (WARM) sx = warm ? (int64_t)pr.template value<u>() : sx;
            if constexpr (MIXED) sx = (is_verb || is_const) ? (int64_t)vv : sx;
            v32 = v32 || sx != (int64_t)(int32_t)sx;
            s = (int32_t)sx;
        } else {
            int32_t sx = (int32_t)((uint32_t)(int32_t)r + (uint32_t)(int32_t)p);
            if constexpr (WARM) sx = warm ? pr.template value<u>() : sx;
            if constexpr (MIXED) sx = (is_verb || is_const) ? vv : sx;
            vmax = max(vmax, sx);
            vmin = min(vmin, sx);
            s = Kind<KIND>::W == 16 ? (int32_t)(int16_t)sx : sx;  // add_inter's InterType wrap
        }
        pr.template push<u>(s);
        if constexpr (PACK16) {
            if constexpr ((u & 1) == 1) pk[(u & 7) >> 1] = pr.template pair<u>();
            if constexpr ((u & 7) == 7) {
                if constexpr (SHIFTS) {
#pragma unroll
                    for (int j = 0; j < 4; j++) pk[j] = pk_shl(pk[j], wasted);
                }
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31 hold channel 0, lanes 32-63 channel 1 of samples i0..i0+7;
                    // after the swaps lanes 0-31 own samples 0-3, lanes 32-63 samples 4-7,
                    // element [0] channel 0 and [1] channel 1
                    const auto a = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
                    const auto b = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
                    uint32_t l0, r0, l1, r1;
                    decorrelate2<DECOR>(a[0], a[1], dm, l0, r0, ovf);
                    decorrelate2<DECOR>(b[0], b[1], dm, l1, r1, ovf);
                    if constexpr (SHIFTS) {
                        l0 = pk_shl(l0, justify);
                        r0 = pk_shl(r0, justify);
                        l1 = pk_shl(l1, justify);
                        r1 = pk_shl(r1, justify);
                    }
                    uint4 v;
                    v.x = __builtin_amdgcn_perm(r0, l0, 0x05040100u);
                    v.y = __builtin_amdgcn_perm(r0, l0, 0x07060302u);
                    v.z = __builtin_amdgcn_perm(r1, l1, 0x05040100u);
                    v.w = __builtin_amdgcn_perm(r1, l1, 0x07060302u);
                    // staged in LDS; the chunk is written back as 128-byte runs per frame
                    sg.put((uint32_t)((u >> 3) & 3), v);
                } else {
                    if constexpr (SHIFTS) {
#pragma unroll
                        for (int j = 0; j < 4; j++) pk[j] = pk_shl(pk[j], justify);
                    }
                    sg.put((uint32_t)((u >> 3) & 3), make_uint4(pk[0], pk[1], pk[2], pk[3]));  // mono: staged
                }
            }
        } else if constexpr (KIND == 2 && LAY != LAY_MULTI) {
            int32_t o = (int32_t)((uint32_t)s << wasted);
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                if constexpr (!wide) big |= (uint32_t)o ^ ((uint32_t)o << 1);
                pair_values(o, x0, x1);
                o = decorrelate<DECOR>(L.chan_code, c1m, x0, x1);
                if (wide) ovf |= decor_overflows<KIND>(L.chan_code, c, x0, x1) ? 1u : 0u;
            }
            pk[u & 7] = (uint32_t)o << justify;
            if constexpr ((u & 7) == 7) {
                const uint32_t i0 = i - 7;
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31: L0..L7, lanes 32-63: R0..R7 -> each half owns 4 L/R pairs
                    const auto a0 = __builtin_amdgcn_permlane32_swap(pk[0], pk[4], false, false);
                    const auto a1 = __builtin_amdgcn_permlane32_swap(pk[1], pk[5], false, false);
                    const auto a2 = __builtin_amdgcn_permlane32_swap(pk[2], pk[6], false, false);
                    const auto a3 = __builtin_amdgcn_permlane32_swap(pk[3], pk[7], false, false);
                    int32_t* dst = reinterpret_cast<int32_t*>(out) + fc.out_elem + 2ull * i0 + (c ? 8 : 0);
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(a0[0], a0[1], a1[0], a1[1]), make_uint4(a2[0], a2[1], a3[0], a3[1]));
                } else {
                    int32_t* dst = reinterpret_cast<int32_t*>(out) + fc.out_elem + i0;
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(pk[0], pk[1], pk[2], pk[3]), make_uint4(pk[4], pk[5], pk[6], pk[7]));
                }
            }
        } else if constexpr (KIND == 0 && LAY != LAY_MULTI) {
            // 8-bit containers, mono / stereo: bytes packed four to a dword, one 16-byte store
            // per 16 samples (per-sample byte stores made every sample a separate L2 write:
            // the 8-bit row ran at 0.015 of HBM). 8-bit samples are never justified, and
            // wasted < 8 here (parse_subframe), so the shift is exact in 32 bits.
            int32_t o = (int32_t)(int8_t)((uint32_t)s << wasted);
            if constexpr (LAY == LAY_STEREO) {
                int32_t x0, x1;
                pair_values(o, x0, x1);
                o = decorrelate<D_GEN>(L.chan_code, c1m, x0, x1);
                ovf |= fits_sb<KIND>(o) ? 0u : 1u;  // exact in i32 for 8-bit values
            }
            if constexpr ((u & 3) == 0) {
                pb = (uint32_t)o;
            } else if constexpr ((u & 3) == 1) {
                pb = __builtin_amdgcn_perm((uint32_t)o, pb, 0x0c0c0400u);  // bytes [s0, s1, 0, 0]
            } else if constexpr ((u & 3) == 2) {
                pb2 = (uint32_t)o;
            } else {
                pk[(u & 15) >> 2] = __builtin_amdgcn_perm(__builtin_amdgcn_perm((uint32_t)o, pb2, 0x0c0c0400u), pb,
                                                          0x05040100u);  // [s0, s1, s2, s3]
            }
            if constexpr ((u & 15) == 15) {
                const uint32_t i0 = i - 15;
                if constexpr (LAY == LAY_STEREO) {
                    // lanes 0-31 hold channel 0, lanes 32-63 channel 1 of samples i0..i0+15: after the
                    // swaps lanes 0-31 own samples 0-7, lanes 32-63 samples 8-15 of both channels
                    const auto a = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
                    const auto b = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
                    uint8_t* dst = reinterpret_cast<uint8_t*>(out) + fc.out_elem + 2ull * i0 + (c ? 16 : 0);
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(__builtin_amdgcn_perm(a[1], a[0], 0x05010400u),
                                    __builtin_amdgcn_perm(a[1], a[0], 0x07030602u),
                                    __builtin_amdgcn_perm(b[1], b[0], 0x05010400u),
                                    __builtin_amdgcn_perm(b[1], b[0], 0x07030602u)),
                         make_uint4(0, 0, 0, 0));
                } else {
                    uint8_t* dst = reinterpret_cast<uint8_t*>(out) + fc.out_elem + i0;
                    emit(std::integral_constant<bool, u == L_ - 1>{}, do_store ? reinterpret_cast<uint4*>(dst) : dummy,
                         make_uint4(pk[0], pk[1], pk[2], pk[3]), make_uint4(0, 0, 0, 0));
                }
            }
        } else {  // 3..8 channels: element stores
            // (wasted < SampleType bits, parse_subframe: a 32-bit shift is exact below 32 bits)
            int32_t o = KIND == 2 ? wrap_st<KIND>((int64_t)((uint64_t)(int64_t)s << wasted))
                                  : wrap_st<KIND>((int64_t)(int32_t)((uint32_t)s << wasted));
            static_assert(LAY == LAY_MULTI, "stereo and mono pack their output above");
            if (do_store) store_elem<KIND>(out, fc.out_elem + (uint64_t)nch * i + c, (int32_t)((uint32_t)o << justify));
        }
    };
    // The ring reads of step s+1 are issued right after step s's consume, before step s's
    // samples (the scheduling fence keeps them there): the samples' arithmetic covers their
    // LDS latency, which would otherwise sit on the bit chain of every step.
    uint32_t whi, wlo;
    rd.fetch(whi, wlo);
    static_for<L_ / NC>([&](auto sc) {
        constexpr int u0 = decltype(sc)::value * NC;
        uint32_t zz[NC];
        int32_t escv = 0;
        int32_t vv = 0;
        uint32_t n;
        const bool warm = WARM && (uint32_t)u0 < wu;
        const uint32_t h = rd.join(whi, wlo);
        if constexpr (MIXED) {
            const uint32_t lim0 = lim;
            n = rice_step<NC, ESC>(h, k, kp1, lim, zz, L.esc, L.escw, escv);
            if constexpr (WARM) n = warm ? 0u : n;
            // a constant enters before its wasted-bits shift: pack-out shifts and wraps it back
            // to L.cval exactly (trunc((cval >> w) << w) = trunc(v << w))
            vv = is_const ? (L.cval >> L.wasted) : ((int32_t)h >> vshift);
            n = is_verb ? (uint32_t)L.cbps : (is_const ? 0u : n);
            lim = (is_verb || is_const) ? lim0 : lim;  // no Rice code in these lanes
            vrange = vrange || (is_verb && !fits_sb<KIND>(vv));
        } else {
            n = rice_step<NC, ESC, RES>(h, k, kp1, lim, zz, L.esc, L.escw, escv);
            if constexpr (WARM) n = warm ? 0u : n;
        }
        rd.consume(n);
        if constexpr (decltype(sc)::value + 1 < L_ / NC) {
            rd.fetch(whi, wlo);
            __builtin_amdgcn_sched_barrier(0x6);  // VALU / SALU may cross, the ring reads may not
        }
        int64_t r0 = RES ? (int64_t)(int32_t)zz[0] : zigzag<KIND>(zz[0]);
        if constexpr (ESC) r0 = L.esc ? (int64_t)escv : r0;
        sample(std::integral_constant<int, u0>{}, r0, warm, vv);
        if constexpr (NC == 2)
            sample(std::integral_constant<int, u0 + 1>{}, RES ? (int64_t)(int32_t)zz[1] : zigzag<KIND>(zz[1]), false, 0);
    });
    const bool dry = rd.dry();  // the ring ran out of stored words: stale reads, redo the chunk
    if constexpr (NC == 1) bad |= lim < L.thr || dry || (MIXED && vrange);
    else bad |= lim > 32u || dry;
    if constexpr (KIND == 2 && LAY == LAY_STEREO && !WIDE) bad |= (int32_t)big < 0 && L.chan_code >= 8;
    if constexpr (KIND == 2) vbad = v32;
    else vbad = vmax > (1 << (Kind<KIND>::SB - 1)) - 1 || vmin < -(1 << (Kind<KIND>::SB - 1));
}

// One chunk in form Form, walked or decoded. A form the kernel lacks is not instantiated and
// runs nothing: run_subframe derives its selectors' compile-time guards from the same in_kernel,
// so the selector of such a form is a constant false and its arm dead code.
template <int KIND, int M, int L_, int LAY, bool MIX, bool WALK, typename Form>
__device__ __forceinline__ void chunk_in_form(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, uint32_t base, const FrameCtx& fc,
                                              void* out, int nch, int c, int32_t c1m, bool lane_fast, uint4* dummy,
                                              bool& bad, Pend& pd, StageOf<LAY>& sg, bool& vbad, uint32_t& ovf,
                                              uint32_t wu) {
    if constexpr (!Form::template in_kernel<KIND, LAY, MIX, WALK>()) return;
    else if constexpr (WALK) walk_chunk<L_, Form>(L, rd, bad, wu);
    else
        fast_chunk<KIND, M, L_, LAY, Form>(L, rd, pr, base, fc, out, nch, c, c1m, lane_fast, dummy, bad, pd, sg, vbad, ovf,
                                           wu);
}

}  // namespace zflac
