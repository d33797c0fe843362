// decode/subframe.h -- lane subframe state; subframe, residual and partition headers; the
// generic (any length) Rice reads; the walk's header pass.
#pragma once
#include "lane_reader.h"
#include "predictor.h"

namespace zflac {

// ----------------------------------------------------------------------------------
// Lane subframe state
// ----------------------------------------------------------------------------------
struct LaneCtx {
    uint32_t bs;
    int bps;           // frame bits per sample
    int ubps;          // + 1 on the side channel (src/zflac.zig:436-441)
    uint32_t chan_code;
    uint32_t end;      // stream end, bit offset from the lane base
    int mode;
    int wasted;
    int cbps;          // coded bits of warm-up / verbatim samples
    int order;
    int shift;
    int32_t cval;
    int method;
    uint32_t psize;
    uint32_t parts_left;
    uint32_t left;     // residuals left in the current partition
    uint32_t k;
    uint32_t kp1;      // k + 1
    uint32_t thr;      // a 32-bit peek below thr means the code is longer than 32 bits
    uint32_t escw;
    bool esc;
    int err;
    // Value-range state (Debug zflac traps, reported as OutOfDomain like the oracle's
    // checked build). `dom`: a predicted sample did not fit the SampleType (:494,537 @intCast)
    // or overflowed the InterType; deferred because zflac reads every residual of a subframe
    // before running its predictor, so a residual read error of the same subframe wins.
    // `unsafe`: the coefficients are large enough that a partial LPC sum could overflow the
    // InterType (sum |c| * 2^(SB-1) over the bound), so the lane takes the generic path, which
    // checks every partial sum in zflac's order (:527-532). `dcr`: decorrelation overflow in
    // the SampleType (:558,564,573-574), reported after the frame's subframes and CRC.
    bool dom;
    bool unsafe;
    uint32_t dcr;
};

// Does v fit the SampleType of container KIND (src/zflac.zig:198-201 @intCast)?
template <int KIND>
__device__ __forceinline__ bool fits_sb(int64_t v) {
    if constexpr (Kind<KIND>::SB == 8) return v == (int64_t)(int8_t)v;
    else if constexpr (Kind<KIND>::SB == 16) return v == (int64_t)(int16_t)v;
    else return v == (int64_t)(int32_t)v;
}
// Largest sum |c| * 2^(SB-1) for which no partial LPC sum can leave the InterType (8-bit:
// i16) and the fast path's i32 `r + prediction` cannot wrap (16-bit: |r| <= 2^30 there).
template <int KIND>
__device__ __forceinline__ constexpr uint64_t safe_lpc_bound() {
    return KIND == 0 ? 0x7FFFull : (KIND == 1 ? (1ull << 30) : ~0ull);
}

__device__ __forceinline__ void set_err(LaneCtx& L, const Rdr& rd, int e) {
    if (!L.err) L.err = (rd.pos() > L.end) ? E_END_OF_STREAM : e;
    L.mode = M_NONE;
}

// Partition header (src/zflac.zig:635-654)
template <int KIND>
__device__ __forceinline__ void read_partition_header(LaneCtx& L, Rdr& rd) {
    const uint32_t k = rd.read(L.method ? 5 : 4);
    L.esc = k == (L.method ? 31u : 15u);
    L.k = L.esc ? 0u : k;
    L.kp1 = L.k + 1;
    L.thr = 1u << L.k;  // q = clz(h) <= 31 - k  <=>  h >= 2^k: the whole code is in the peek
    L.escw = 0;
    if (L.esc) {
        L.escw = rd.read(5);
        if (L.escw > (uint32_t)Kind<KIND>::W) set_err(L, rd, E_OUT_OF_DOMAIN);  // read_signed_integer assert
    } else if (k >= (uint32_t)Kind<KIND>::W) {
        set_err(L, rd, E_OUT_OF_DOMAIN);  // :656 unreachable
    }
    L.left = L.psize;
    L.parts_left--;
}

// Residual header (src/zflac.zig:614-633)
template <int KIND>
__device__ __forceinline__ void read_residual_header(LaneCtx& L, Rdr& rd) {
    const uint32_t method = rd.read(2);
    if (method >= 2) { set_err(L, rd, E_INVALID_RESIDUAL_CODING); return; }  // :618
    L.method = (int)method;
    const uint32_t po = rd.read(4);
    L.psize = L.bs >> po;
    // :626 `count -= order` underflow; :623-632 stale residuals when bs % 2^po != 0
    if (L.psize < (uint32_t)L.order || (L.psize << po) != L.bs) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
    L.parts_left = 1u << po;
    read_partition_header<KIND>(L, rd);
    L.left = L.psize - (uint32_t)L.order;
}

template <int KIND>
__device__ __forceinline__ int64_t zigzag(uint64_t zz) {
    if constexpr (Kind<KIND>::W == 64) return (int64_t)((zz >> 1) ^ (0 - (zz & 1)));
    else if constexpr (Kind<KIND>::W == 32) return (int32_t)(((uint32_t)zz >> 1) ^ (0u - ((uint32_t)zz & 1)));
    else {
        const uint32_t z = (uint32_t)zz & 0xFFFFu;
        return (int16_t)((z >> 1) ^ (0u - (z & 1)));
    }
}

// Rice code, any length (src/zflac.zig:657-663)
template <int KIND>
__device__ __forceinline__ int64_t rice_general(LaneCtx& L, Rdr& rd) {
    uint32_t q;
    if (!rd.unary(L.end, q)) { set_err(L, rd, E_END_OF_STREAM); return 0; }
    const uint32_t rem = rd.read(L.k);
    if constexpr (Kind<KIND>::W == 16) {
        if (q > 0xFFFFu) set_err(L, rd, E_OUT_OF_DOMAIN);  // @intCast(readUnary()) to u16
    }
    if constexpr (Kind<KIND>::W == 64) return zigzag<KIND>(((uint64_t)q << L.k) + rem);
    else return zigzag<KIND>((uint64_t)((q << L.k) + rem));  // `<<` discards in u32 / u16
}

// One residual of the current partition, generic path.
template <int KIND>
__device__ __forceinline__ int64_t residual_general(LaneCtx& L, Rdr& rd) {
    if (L.esc) return L.escw ? (int64_t)rd.read_signed(L.escw) : 0;
    const uint32_t h = rd.hi();
    if (h >= L.thr) {
        const uint32_t q = __builtin_clz(h);
        const uint32_t len = q + L.kp1;
        const uint32_t rem = __builtin_amdgcn_ubfe(h, 32 - len, L.k);
        rd.consume(len);
        return zigzag<KIND>((q << L.k) | rem);
    }
    return rice_general<KIND>(L, rd);
}

// Warm-up samples (src/zflac.zig:474,506 read_unencoded_sample): each must fit the
// SampleType, checked as it is read; the first that does not ends the subframe there.
template <int KIND, int M>
__device__ __forceinline__ bool read_warmup(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr, int order) {
    bool ok = true;
    static_for<M>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if (J < order && ok) {
            rd.ensure(3);
            const int64_t v = rd.read_signed_wide((uint32_t)L.cbps);
            ok = fits_sb<KIND>(v);
            pr.template push<J>((int32_t)v);
        }
    });
    if (!ok) set_err(L, rd, E_OUT_OF_DOMAIN);
    return ok;
}

// Full subframe header (src/zflac.zig:426-520); warm-up samples are pushed as samples
// 0..order-1 of the predictor history.
template <int KIND, int M>
__device__ __forceinline__ void parse_subframe(LaneCtx& L, Rdr& rd, Pred<KIND, M>& pr) {
    L.mode = M_NONE;
    L.unsafe = false;
    pr.clear();
    const uint32_t h8 = rd.read(8);
    if (h8 >> 7) { set_err(L, rd, E_INVALID_SUBFRAME_HEADER); return; }  // :431
    const uint32_t type = (h8 >> 1) & 63;
    int wasted = 0;
    if (h8 & 1) {  // :433
        uint32_t u;
        if (!rd.unary(L.end, u)) { set_err(L, rd, E_END_OF_STREAM); return; }
        if (u + 1 >= 64) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        wasted = (int)u + 1;
    }
    L.wasted = wasted;
    if (type == 0) {  // constant: reads bits_per_sample, not the side depth (:447)
        if (L.bps <= wasted || L.bps - wasted > Kind<KIND>::W || wasted >= Kind<KIND>::SB) {
            set_err(L, rd, E_OUT_OF_DOMAIN);
            return;
        }
        const int64_t v = rd.read_signed_wide((uint32_t)(L.bps - wasted));
        if (!fits_sb<KIND>(v)) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }  // rd_unencoded @intCast
        L.cval = wrap_st<KIND>((int64_t)((uint64_t)v << wasted));
        L.mode = M_CONST;
        return;
    }
    if (L.ubps <= wasted || L.ubps - wasted > Kind<KIND>::W || (wasted > 0 && wasted >= Kind<KIND>::SB)) {
        set_err(L, rd, E_OUT_OF_DOMAIN);
        return;
    }
    L.cbps = L.ubps - wasted;
    if (type == 1) {  // verbatim (:455-465)
        L.mode = M_VERB;
        return;
    }
    int order;
    if (type >= 8 && type <= 12) {  // fixed (:466-490) as LPC with shift 0
        order = (int)type - 8;
        L.shift = 0;
        if (!read_warmup<KIND, M>(L, rd, pr, order)) return;
        if (order == 1) pr.template set_coef<0>(1);
        if (order == 2) {
            pr.template set_coef<0>(2);
            pr.template set_coef<1>(-1);
        }
        if (order == 3) {
            pr.template set_coef<0>(3);
            pr.template set_coef<1>(-3);
            pr.template set_coef<2>(1);
        }
        if (order == 4) {
            pr.template set_coef<0>(4);
            pr.template set_coef<1>(-6);
            pr.template set_coef<2>(4);
            pr.template set_coef<3>(-1);
        }
    } else if (type >= 32) {  // LPC (:499-520)
        order = (int)type - 31;
        if (!read_warmup<KIND, M>(L, rd, pr, order)) return;
        rd.ensure(2);
        const uint32_t pc = rd.read(4);
        if (pc == 15) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }  // u4 `+ 1` overflow (:508)
        const uint32_t prec = pc + 1;
        L.shift = (int)rd.read(5);  // unsigned u5 (:510)
        if (L.shift >= Kind<KIND>::W) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        uint64_t sum_abs = 0;
        static_for<M>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if (J < order) {
                rd.ensure(2);
                const int32_t cf = rd.read_signed(prec);
                sum_abs += (uint64_t)(cf < 0 ? -(int64_t)cf : cf);
                pr.template set_coef<J>(cf);
            }
        });
        L.unsafe = (sum_abs << (Kind<KIND>::SB - 1)) > safe_lpc_bound<KIND>();
    } else {
        set_err(L, rd, E_INVALID_SUBFRAME_HEADER);  // reserved (:542)
        return;
    }
    L.order = order;
    rd.ensure(2);
    read_residual_header<KIND>(L, rd);
    if (L.err) return;
    L.mode = M_PRED;
}

// Walk: same reads as parse_subframe + residuals, no samples (src/zflac.zig:426-541).
template <int KIND>
__device__ __forceinline__ void walk_subframe(LaneCtx& L, Rdr& rd) {
    const uint32_t h8 = rd.read(8);
    if (h8 >> 7) { set_err(L, rd, E_INVALID_SUBFRAME_HEADER); return; }
    const uint32_t type = (h8 >> 1) & 63;
    int wasted = 0;
    if (h8 & 1) {
        uint32_t u;
        if (!rd.unary(L.end, u)) { set_err(L, rd, E_END_OF_STREAM); return; }
        if (u + 1 >= 64) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        wasted = (int)u + 1;
    }
    if (type == 0) {
        if (L.bps <= wasted) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        rd.skip((uint32_t)(L.bps - wasted));
        L.mode = M_NONE;  // done
        return;
    }
    if (L.ubps <= wasted) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
    const uint32_t cb = (uint32_t)(L.ubps - wasted);
    if (type == 1) {
        rd.skip((uint64_t)L.bs * cb);
        L.mode = M_NONE;  // done
        return;
    }
    int order;
    if (type >= 8 && type <= 12) {
        order = (int)type - 8;
        rd.skip((uint64_t)order * cb);
    } else if (type >= 32) {
        order = (int)type - 31;
        rd.skip((uint64_t)order * cb);
        rd.ensure(2);
        const uint32_t pc = rd.read(4);
        if (pc == 15) { set_err(L, rd, E_OUT_OF_DOMAIN); return; }
        rd.read(5);
        rd.skip((uint64_t)order * (pc + 1));
    } else {
        set_err(L, rd, E_INVALID_SUBFRAME_HEADER);
        return;
    }
    L.order = order;
    rd.ensure(2);
    read_residual_header<KIND>(L, rd);
    L.mode = L.err ? M_NONE : M_PRED;
}

}  // namespace zflac
