// dspi_chain_pk.inc — the float (RP2350) chain with TWO streams per lane on packed FP32 (v_pk_mul_f32 / v_pk_add_f32).
// Included by dspi_kernels.hip inside its anonymous namespace.
//
// Why: the float chain is VALU-issue bound (a SIMD issues one vector instruction per ~4.1 cycles whatever the
// occupancy, tools/probe/probe3), and a VOP3P packed-f32 instruction does two independent IEEE multiplies/adds in one
// issue slot (tools/probe/probe4).  Lane l of a workgroup carries streams 2l and 2l+1 of the workgroup's 128-stream
// row as the two halves of a 64-bit VGPR pair; both halves see the same parameter image (the host only sends lanes
// whose two streams share an image here, the rest go through the one-stream kernel, component by component).
// Every arithmetic step is the same single IEEE operation as in the one-stream kernel, so results are bit-identical.
//
// Reference path: as dspi_kernels.hip (usb_audio.c:560-967, dsp_pipeline.c:281-365, leveller.c:148-261, crossfeed.c:132-156).

typedef float v2f __attribute__((ext_vector_type(2)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// development switches (stream-major emission; timing only, WRONG words unless noted): -DDSPI_EXP_EMIT=1 no emission stores, 2 no emission loads,
// 16 (right words) the previous step's rows drained at the END of the step behind the step's own stores instead of after the EQ — no effect
// (profiles/r04_headline_experiments.md)
#ifndef DSPI_EXP_EMIT
#define DSPI_EXP_EMIT 0
#endif
// Stream-major words: the S/PDIF pairs (bit p = pair p) whose emission the master SIMD's third wave takes over from the pair's own two waves
// (pair_emit_load / pair_emit_finish below; 0: every pair emits its own halves).  Pair 3 = outputs 6 and 7, the third waves of the first
// two output SIMDs (pk_role); pair 2 = outputs 4 and 5.  0xC: 9.93 -> 9.78 ms on one box against 9.92 for 0x8 and 9.78 for 0xA
// (profiles/r05_headline_experiments.md).
#ifndef DSPI_EMIT_PAIRS
#define DSPI_EMIT_PAIRS 0xC
#endif
constexpr uint32_t ROWP = 128;                      // streams per workgroup row
constexpr int HALF = 64;                            // v2f elements per row
constexpr int kMailbox = 8;                         // packets of leveller gain in flight between the two master waves

__device__ __forceinline__ v2f as_v2f(v2u u) { return __builtin_bit_cast(v2f, u); }
__device__ __forceinline__ v2u as_v2u(v2f f) { return __builtin_bit_cast(v2u, f); }
__device__ __forceinline__ v2f splat(float f) { return v2f{f, f}; }
// clamp to [-1, 1] (usb_audio.c:926-941) as the median of {x, -1, 1}: one instruction; equal to the reference's two
// comparisons for every non-NaN x (a NaN has no defined word in the reference either: its (int32_t) cast is undefined)
__device__ __forceinline__ float clamp_pm1(float x) {
    float r;
    asm("v_med3_f32 %0, %1, -1.0, 1.0" : "=v"(r) : "v"(x));
    return r;
}
// pk = (|x| > pk) ? |x| : pk   (pk is never NaN; a NaN x leaves pk alone in both forms)
__device__ __forceinline__ float peak_acc(float pk, float x) { asm("v_max_f32 %0, |%1|, %0" : "+v"(pk) : "v"(x)); return pk; }
// two samples per instruction: max is associative and exact, so max3(pk, |a|, |b|) is the same meter value
__device__ __forceinline__ float peak_acc2(float pk, float a, float b) { asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pk) : "v"(a), "v"(b)); return pk; }

// ragged chunk: sample i of n counts only if i < n (wave-uniform select; compiled out of the kernels for even packets)
__device__ __forceinline__ v2f live(v2f v, bool tail, int i, int n) { return (tail && i >= n) ? v2f{0.0f, 0.0f} : v; }

struct __attribute__((aligned(32))) DevBandPk {     // DevBand seen as three aligned coefficient pairs
    v2f c01, c23, c45;
    uint32_t kind, pad;
};
static_assert(sizeof(DevBandPk) == sizeof(DevBand), "DevBand view");
typedef const __attribute__((address_space(4))) DevBandPk *BandPkPtr;

#include "dspi_bandloops_pk.inc"
#include "dspi_bandloops_pk_fma.inc"
#include "dspi_bandloops_pkv.inc"
#include "dspi_bandloops_pkv_fma.inc"

// a*b + c under the context's float contract (include/dspi.h DSPI_FLOAT_CONTRACT_FMA): FMA = the firmware build's fused
// multiply-add (one rounding, v_pk_fma_f32), otherwise the two roundings of the source read literally (-ffp-contract=off).
// Every use below is one of the statements GCC contracts in the reference (DESIGN.md section 5 lists them with their source lines).
template <bool FMA> __device__ __forceinline__ v2f mad2(v2f a, v2f b, v2f c) {
    if (FMA) return __builtin_elementwise_fma(a, b, c);
    return a * b + c;
}
template <bool FMA> __device__ __forceinline__ v2f mad2(float a, v2f b, v2f c) { return mad2<FMA>(splat(a), b, c); }
// A per-lane number that multiplies all sixteen samples of a chunk: defined HERE, inside the time loop.  Used straight from its
// launch-invariant register, every one of the sixteen packed multiply-adds gets its own hoisted copy of it (32 registers, or scratch:
// tools/scratch_map.py found 34 scratch instructions per step in the output waves of the per-lane-filter kernel from this alone).
__device__ __forceinline__ v2f here(v2f v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ float here(float v) { return v; }      // (a uniform number is an SGPR operand of the instruction)

// ---- per-lane values (PV): rows whose streams carry different presets of ONE structure (dspi_image.h, value tile) ----
// A number that the shared-preset kernel reads from the workgroup's image with a scalar load (float, broadcast to the lane's two
// streams by the instruction) is, with PV, a v2f {stream a, stream b} read from the row's value tile: one coalesced 512-byte
// row per wave.  Everything that steers control flow (flags, kinds, bypasses, enables, delays) still comes from the image.
template <bool PV> struct PvT { typedef float type; };
template <> struct PvT<true> { typedef v2f type; };
template <bool PV>
__device__ __forceinline__ typename PvT<PV>::type pv_val(const float *tile, uint32_t lane, int idx, float uniform) {
    if constexpr (PV) return *reinterpret_cast<const v2f *>(tile + kPvBandFloats + (idx * kLanes + (int)lane) * 2);
    else return uniform;
}
__device__ __forceinline__ float pv_c(float v, int) { return v; }
__device__ __forceinline__ float pv_c(v2f v, int c) { return v[c]; }

// ---- [position][128] arrays in HBM (leveller ring planes, delay lines): the lane's two columns ----
// `base` is the wave-uniform start of the array (SGPR pair), `lo` the lane's word offset (2*lane): accesses are
// SGPR base + 32-bit VGPR offset, so no 64-bit per-row pointers are kept in VGPRs.
// Fast path: both streams at the same position and no wrap inside the chunk -> one 8-byte access per row (a 512-byte
// coalesced row per wave).  Streams whose positions have drifted apart (different histories of "delay active" /
// "leveller on" before they came to share an image) take the general per-stream path.
// Ragged chunks (TAIL, n < T): loads always fetch all T rows — positions wrap, so the extra rows are valid memory and
// their values are never used — because a sample array that is WRITTEN under an early exit costs hipcc hundreds of
// register copies and spills; stores stop at n (uniform branches between stores touch no registers).
// OTHER_WAVE: the rows were written by a different wave of this workgroup (the leveller ring between the two master
// waves).  Those loads go to the device-coherent level (agent-scope relaxed atomic loads: sc1) instead of trusting the
// CU's vector L1 for lines this wave may have cached one ring revolution ago.
__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ v2u ld_agent2(const uint32_t *p) {
    const uint64_t w = __hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v2u{(uint32_t)w, (uint32_t)(w >> 32)};
}
template <bool TAIL, bool OTHER_WAVE = false, int R = T>
__device__ __forceinline__ void rows_load(v2f (&d)[R], int n, const uint32_t *base, uint32_t lo, v2u p, uint32_t pmask) {
    if (__all(p.x == p.y && p.x + R <= pmask + 1u)) {
        WT_COUNT(OTHER_WAVE ? 4 : 0, lo);
        const uint32_t off = p.x * ROWP + lo;
#pragma unroll
        for (int i = 0; i < R; ++i)
            d[i] = as_v2f(OTHER_WAVE ? ld_agent2(base + (off + i * ROWP)) : *reinterpret_cast<const v2u *>(base + (off + i * ROWP)));
    } else {
        WT_COUNT(OTHER_WAVE ? 5 : 1, lo);
        uint32_t px = p.x, py = p.y;
        asm volatile("" : "+v"(px), "+v"(py));     // opaque here: keeps the 32 offsets of this cold path from being hoisted (and spilled)
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t *qx = base + (((px + i) & pmask) * ROWP + lo), *qy = base + (((py + i) & pmask) * ROWP + lo + 1);
            d[i].x = as_f(OTHER_WAVE ? ld_agent(qx) : *qx);
            d[i].y = as_f(OTHER_WAVE ? ld_agent(qy) : *qy);
        }
    }
}
template <bool TAIL, bool NT = false>
__device__ __forceinline__ void rows_store(const v2f (&d)[T], int n, uint32_t *base, uint32_t lo, v2u p, uint32_t pmask) {
    if (__all(p.x == p.y && p.x + T <= pmask + 1u)) {
        WT_COUNT(2, lo);
        const uint32_t off = p.x * ROWP + lo;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (TAIL && i >= n) continue;
            if (NT) __builtin_nontemporal_store(as_v2u(d[i]), reinterpret_cast<v2u *>(base + (off + i * ROWP)));
            else *reinterpret_cast<v2u *>(base + (off + i * ROWP)) = as_v2u(d[i]);
        }
    } else {
        WT_COUNT(3, lo);
        uint32_t px = p.x, py = p.y;
        asm volatile("" : "+v"(px), "+v"(py));
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (TAIL && i >= n) continue;
            base[((px + i) & pmask) * ROWP + lo] = as_u(d[i].x);
            base[((py + i) & pmask) * ROWP + lo + 1] = as_u(d[i].y);
        }
    }
}

// ---- EQ bands ----
// full-chunk runner on the list-scheduled loops; band b+1's coefficients (scalar loads) and state (LDS) are
// requested before band b's arithmetic starts (see run_bands16)
template <int NB, bool RAGGED = false, bool FMA = false>
__device__ __forceinline__ void run_bands16_pk(v2f (&x)[T], BandPtr bands_, v2f *__restrict__ st, uint32_t n = T) {
    BandPkPtr bands = reinterpret_cast<BandPkPtr>(bands_);
    uint32_t kind = bands[0].kind;
    v2f c01 = bands[0].c01, c23 = bands[0].c23, c45 = bands[0].c45;
    v2f s1 = st[0], s2 = st[HALF];
    asm volatile("" ::"s"(kind), "s"(c01), "s"(c23), "s"(c45), "v"(s1), "v"(s2));
#pragma unroll 2
    for (int b = 0; b < NB; ++b) {
        const int bn = (b + 1 < NB) ? b + 1 : b;
        BandPkPtr nb = bands + bn;
        const uint32_t nkind = nb->kind;
        const v2f n01 = nb->c01, n23 = nb->c23, n45 = nb->c45;
        const v2f ns1 = st[bn * 2 * HALF], ns2 = st[bn * 2 * HALF + HALF];
        if (RAGGED) {      // kernels for ragged packets: one statement for full and short chunks
            if (FMA) band16pkf_any_n(x, s1, s2, kind, c01, c23, c45, n); else band16pk_any_n(x, s1, s2, kind, c01, c23, c45, n);
        } else if (FMA) band16pkf_any(x, s1, s2, kind, c01, c23, c45);
        else band16pk_any(x, s1, s2, kind, c01, c23, c45);
        st[b * 2 * HALF] = s1;
        st[b * 2 * HALF + HALF] = s2;
        kind = nkind; c01 = n01; c23 = n23; c45 = n45; s1 = ns1; s2 = ns2;
    }
}

// Two channels at once (master intake: left + right).  A single channel's recurrences are latency-bound — a biquad's
// s1 -> y -> a1*y -> ... -> s1 loop is four dependent packed ops, ~64 cycles per sample against 36 cycles of issue — and
// the intake wave has most of its SIMD to itself, so its 24 band visits per chunk used to set a floor under the whole
// step.  Bands whose kinds agree in both channels (the usual stereo EQ) run the interleaved loops (band16pk2_*); a pair
// with different kinds runs channel by channel inside the same asm statement.  on_a / on_b: channel not bypassed.
template <int NB, bool SHELF_ONLY, bool RAGGED, bool FMA>
__device__ __forceinline__ void run_bands16_pk2(v2f (&xa)[T], v2f (&xb)[T], BandPtr ba_, BandPtr bb_, bool on_a, bool on_b,
                                                v2f *__restrict__ sta, v2f *__restrict__ stb, uint32_t n) {
    BandPkPtr ba = reinterpret_cast<BandPkPtr>(ba_), bb = reinterpret_cast<BandPkPtr>(bb_);
    uint32_t ka = on_a ? ba[0].kind : 0u, kb = on_b ? bb[0].kind : 0u;
    v2f a01 = ba[0].c01, a23 = ba[0].c23, a45 = ba[0].c45, b01 = bb[0].c01, b23 = bb[0].c23, b45 = bb[0].c45;
    v2f s1a = sta[0], s2a = sta[HALF], s1b = stb[0], s2b = stb[HALF];
    asm volatile("" ::"s"(ka), "s"(kb), "s"(a01), "s"(a23), "s"(a45), "s"(b01), "s"(b23), "s"(b45), "v"(s1a), "v"(s2a), "v"(s1b), "v"(s2b));
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        const int bn = (b + 1 < NB) ? b + 1 : b;
        const uint32_t nka = on_a ? ba[bn].kind : 0u, nkb = on_b ? bb[bn].kind : 0u;
        const v2f na01 = ba[bn].c01, na23 = ba[bn].c23, na45 = ba[bn].c45, nb01 = bb[bn].c01, nb23 = bb[bn].c23, nb45 = bb[bn].c45;
        const v2f ns1a = sta[bn * 2 * HALF], ns2a = sta[bn * 2 * HALF + HALF], ns1b = stb[bn * 2 * HALF], ns2b = stb[bn * 2 * HALF + HALF];
        if (FMA) {
            if (RAGGED) {
                if (SHELF_ONLY) band16pk2f_shelf_n(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45, n);
                else band16pk2f_any_n(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45, n);
            } else if (SHELF_ONLY) band16pk2f_shelf(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45);
            else band16pk2f_any(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45);
        } else if (RAGGED) {       // kernels for ragged packets: a short chunk runs channel a, then channel b, inside the same statement
            if (SHELF_ONLY) band16pk2_shelf_n(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45, n);
            else band16pk2_any_n(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45, n);
        } else if (SHELF_ONLY) band16pk2_shelf(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45);
        else band16pk2_any(xa, xb, s1a, s2a, s1b, s2b, ka, kb, a01, a23, a45, b01, b23, b45);
        sta[b * 2 * HALF] = s1a; sta[b * 2 * HALF + HALF] = s2a;
        stb[b * 2 * HALF] = s1b; stb[b * 2 * HALF + HALF] = s2b;
        ka = nka; kb = nkb; a01 = na01; a23 = na23; a45 = na45; b01 = nb01; b23 = nb23; b45 = nb45;
        s1a = ns1a; s2a = ns2a; s1b = ns1b; s2b = ns2b;
    }
}

// per-lane coefficients: band slot `slot0 + b` of the row's value tile, three 16-byte loads per lane and band (coalesced), the
// next band's requested before this band's arithmetic starts; kinds (wave-uniform) from the image as before
struct PvCoef { v2f c0, c1, c2, c3, c4, c5; };
// (only what the band's form reads is fetched: nothing for a bypassed band, c4 / c5 for the biquad and the shelf only — the value
//  tiles are most of this kernel's HBM traffic, DESIGN.md section 6)
__device__ __forceinline__ PvCoef pv_band(const float *tile, uint32_t lane, int slot, uint32_t kind) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    // wave-uniform base (scalar arithmetic) + the lane's 32-bit byte offset: a 64-bit per-lane address per band is loop-invariant, gets
    // hoisted out of the time loop for all ten bands of the channel and lives in scratch (the callers pass an opaque copy of the lane index)
    const f4 *p = reinterpret_cast<const f4 *>(reinterpret_cast<const char *>(tile) + (size_t)(uint32_t)slot * (3 * kLanes * 16) + (size_t)(lane * 16u));
    PvCoef k;
    k.c0 = k.c1 = k.c2 = k.c3 = k.c4 = k.c5 = v2f{0.0f, 0.0f};
    if (kind != K_BYPASS) {
        const f4 a = p[0], b = p[kLanes];
        k.c0 = v2f{a.x, a.y}; k.c1 = v2f{a.z, a.w}; k.c2 = v2f{b.x, b.y}; k.c3 = v2f{b.z, b.w};
        k.c4 = k.c2; k.c5 = k.c3;                  // not read by the forms that skip the third load
        if (kind == K_BIQUAD || kind == K_SVF_SHELF) { const f4 c = p[2 * kLanes]; k.c4 = v2f{c.x, c.y}; k.c5 = v2f{c.z, c.w}; }
    }
    return k;
}
template <bool FMA, bool RAGGED>
__device__ __forceinline__ void pv_band_run(v2f (&x)[T], v2f &s1, v2f &s2, uint32_t kind, const PvCoef &k, uint32_t n) {
    if (RAGGED) {
        if (FMA) band16pkvf_any_n(x, s1, s2, kind, k.c0, k.c1, k.c2, k.c3, k.c4, k.c5, n);
        else band16pkv_any_n(x, s1, s2, kind, k.c0, k.c1, k.c2, k.c3, k.c4, k.c5, n);
    } else if (FMA) band16pkvf_any(x, s1, s2, kind, k.c0, k.c1, k.c2, k.c3, k.c4, k.c5);
    else band16pkv_any(x, s1, s2, kind, k.c0, k.c1, k.c2, k.c3, k.c4, k.c5);
}
// The next band's coefficients are requested before this band's arithmetic starts.  Tried again in round 3, with the scratch gone from
// the output loop (DESIGN.md section 6.0): two bands of look-ahead — 1 % on the one-band case, 2-8 % SLOWER when every band differs (12
// more live registers); bands that do not differ between the row's streams served from the image's scalars, broadcast into the
// registers this loop reads (one loop body, a uniform branch per band around the loads) — the one-master-band case gains 7 %, one output
// band per stream loses 5 %, every band 9 % (the output loop picks up 26 scratch instructions per step from a change in the master code).
template <int NB, bool FMA, bool RAGGED>
__device__ __forceinline__ void run_bands16_pkv(v2f (&x)[T], BandPtr bands, bool on, const float *tile, int slot0, uint32_t lane, v2f *__restrict__ st, uint32_t n) {
    uint32_t kind = on ? bands[0].kind : 0u;
    asm volatile("" : "+v"(lane));      // see pv_band
    PvCoef cur = pv_band(tile, lane, slot0, kind);
    v2f s1 = st[0], s2 = st[HALF];
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        const int bn = (b + 1 < NB) ? b + 1 : b;
        const uint32_t nkind = on ? bands[bn].kind : 0u;
        const PvCoef nxt = pv_band(tile, lane, slot0 + bn, nkind);
        const v2f ns1 = st[bn * 2 * HALF], ns2 = st[bn * 2 * HALF + HALF];
        pv_band_run<FMA, RAGGED>(x, s1, s2, kind, cur, n);
        st[b * 2 * HALF] = s1;
        st[b * 2 * HALF + HALF] = s2;
        kind = nkind; cur = nxt; s1 = ns1; s2 = ns2;
    }
}
// Which of `nb` bands from slot `slot0` differ between the row's streams (value-tile mask, built with the tile; wave-uniform).  A
// CHANNEL none of whose bands differ — the usual state of most channels of a product family's presets — takes the image's scalars
// and the shared-preset loops: no tile traffic for it.  (Per band instead of per channel was tried: both loops in one band loop cost
// the allocator more than the traffic saved.)
__device__ __forceinline__ uint32_t pv_differ(const float *tile, int slot0, int nb) {
    const uint32_t *m = reinterpret_cast<const uint32_t *>(tile + kPvMaskWord);
    const uint32_t w = (uint32_t)slot0 >> 5, sh = (uint32_t)slot0 & 31u;
    const uint64_t two = (uint64_t)__builtin_amdgcn_readfirstlane(m[w]) | ((uint64_t)__builtin_amdgcn_readfirstlane(m[w + 1 < 4 ? w + 1 : 3]) << 32);
    return (uint32_t)(two >> sh) & ((1u << nb) - 1u);
}

template <bool TAIL, int NB, bool FMA>
__device__ __forceinline__ void run_bands_pk(v2f (&x)[T], int n, BandPtr bands, v2f *__restrict__ st) {
    // ragged packets (44/45 frames): only the last chunk of a packet is short; the full ones take the scheduled loops too
    // (the choice is made inside the asm statement, see tools/gen_bandloops.py emit_n)
    run_bands16_pk<NB, TAIL, FMA>(x, bands, st, (uint32_t)n);
}

// ==========================================================================================
// master wave
// ==========================================================================================
struct MasterPk {
    v2f lpL, lpR, apL, apR;
    v2f env_l, env_r, gsm_db, g_cur, g_prev;
    v2u rp1, rp2;
    v2f p2_gain, p2_step, g_last;            // g_last: gain at the end of the previous packet's ramp (hand-off wave)
    v2f pk_l, pk_r;
    v2u clip;
    u32x4 pre[2][T / 4];
    uint32_t pre_valid;
};

__device__ __forceinline__ void pcm16_to_f(const u32x4 (&w)[T / 4], int c, v2f (&xl)[T], v2f (&xr)[T]) {
#pragma unroll
    for (int v = 0; v < T / 4; ++v)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xl[v * 4 + e][c] = (float)(int32_t)(int16_t)(w[v][e] & 0xffffu);
            xr[v * 4 + e][c] = (float)((int32_t)w[v][e] >> 16);
        }
}

// One step of the master wave.  With the leveller on, chunk q = (kq, cq) leaves the wave one packet after it entered
// (pass 1 of packet k, pass 2 of packet k-1, see dspi_kernels.hip), and the two halves of a step are independent:
// the hand-off half runs FIRST on ring rows that were requested at the end of the previous step (m.o_l / m.o_r), the
// intake half second, so the 2 x 32 sample registers are shared by both and the ring latency hides behind the barrier.
// With the leveller off the hand-off consumes what the intake half of the same step produced.
template <bool TAIL, bool FMA, bool PV>
__device__ __forceinline__ void master_handoff_pk(const KArgs &a, ImgPtr img, const float *tile, const StateMap &sm, const Geo &g, MasterPk &m,
                                                  v2f (&xl)[T], v2f (&xr)[T], v2f *__restrict__ xch_base, const v2f *__restrict__ mailbox,
                                                  uint32_t wg, uint32_t lane, uint32_t stream, bool lev_on, uint32_t kq, uint32_t cq, uint32_t q) {
    const uint32_t flags = img->flags;
    const int nq = TAIL ? (int)min((uint32_t)T, g.B - cq * T) : T;
    if (lev_on) {
        if (cq == 0) {   // ramp of packet kq (leveller.c:208-216): from the previous packet's gain to the one the intake wave
                         // decided when pass 1 of packet kq ended (posted in the LDS mailbox at least one barrier ago)
            const v2f g_new = mailbox[(kq & (kMailbox - 1)) * HALF + lane];
            if (g.B == 1) { m.p2_gain = g_new; m.p2_step = splat(0.0f); }
            else { m.p2_step = (g_new - m.g_last) / (float)(g.B - 1); m.p2_gain = m.g_last; }
            m.g_last = g_new;
        }
        // ---- leveller pass 2: interpolated gain, lookahead, gain-cap limiter (leveller.c:208-261) ----
        // The limiter only acts where gain > 1 (leveller.c:236).  The ramp is linear, so if neither end of this chunk
        // exceeds 1 for any stream of the wave the whole test is skipped; otherwise it runs branch-free (the quotient is
        // formed for every sample and selected exactly where the reference would have used it).
        const float ceil_ = 0.70795f;
        const v2f g_end = m.p2_gain + m.p2_step * (float)T;     // bound only, not used in the arithmetic
        const bool limiter = __any(m.p2_gain.x > 1.0f || m.p2_gain.y > 1.0f || g_end.x > 1.0f || g_end.y > 1.0f ||
                                   !(g_end.x == g_end.x) || !(g_end.y == g_end.y));
        // ragged chunk: all T samples are scaled (the extra ones are never used), the ramp value after nq steps is kept
        v2f gain_n = m.p2_gain;
        if (limiter) {
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (TAIL && i == nq) gain_n = m.p2_gain;
                v2f gg = m.p2_gain;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    float peak = fabsf(xl[i][c]);
                    const float pr = fabsf(xr[i][c]);
                    if (pr > peak) peak = pr;
                    const float g1 = gg[c];
                    const float mg = ceil_ / peak;
                    const float capped = (mg > 1.0f) ? mg : 1.0f;
                    const bool use = (peak > 0.0f) && (g1 > 1.0f) && (mg < g1);
                    gg[c] = use ? capped : g1;
                }
                xl[i] = xl[i] * gg;
                xr[i] = xr[i] * gg;
                m.p2_gain += m.p2_step;
            }
        } else {
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (TAIL && i == nq) gain_n = m.p2_gain;
                xl[i] = xl[i] * m.p2_gain;
                xr[i] = xr[i] * m.p2_gain;
                m.p2_gain += m.p2_step;
            }
        }
        if (TAIL && nq != T) m.p2_gain = gain_n;      // the ramp advanced nq times
        if (cq == g.cpb - 1) m.rp2 = (m.rp2 + g.B) & (uint32_t)(kRingLen - 1);
    }
    // ---- master peaks (pre-crossfeed) + crossfeed (usb_audio.c:741-749, crossfeed.c:132-156) ----
    if (cq == 0) { m.pk_l = splat(0.0f); m.pk_r = splat(0.0f); }
    const bool xf = flags & IF_CROSSFEED_ON;
    // (per-lane values: the tile offsets are formed here, per step, from an opaque copy of the lane index — hoisted out of the time loop they
    //  live in scratch, one per value)
    uint32_t lane_v = lane;
    if constexpr (PV) asm volatile("" : "+v"(lane_v));
    const auto a0 = here(pv_val<PV>(tile, lane_v, PV_XF + 0, img->xf_lp_a0.f)), b1 = here(pv_val<PV>(tile, lane_v, PV_XF + 1, img->xf_lp_b1.f)),
               apa = here(pv_val<PV>(tile, lane_v, PV_XF + 2, img->xf_ap_a.f));
    v2f *xch = xch_base + (size_t)(q & 1u) * (2 * T * HALF) + lane;
#pragma unroll
    for (int i = 0; i < T; i += 2) {      // ragged chunk: samples past nq count as 0 (no early exits, see rows_load)
        const v2f l0 = live(xl[i], TAIL, i, nq), l1 = live(xl[i + 1], TAIL, i + 1, nq), r0 = live(xr[i], TAIL, i, nq), r1 = live(xr[i + 1], TAIL, i + 1, nq);
#pragma unroll
        for (int c = 0; c < 2; ++c) { m.pk_l[c] = peak_acc2(m.pk_l[c], l0[c], l1[c]); m.pk_r[c] = peak_acc2(m.pk_r[c], r0[c], r1[c]); }
    }
    v2f n_lpL = m.lpL, n_lpR = m.lpR, n_apL = m.apL, n_apR = m.apR;      // ragged chunk: the filter state after nq samples
#pragma unroll
    for (int i = 0; i < T; ++i) {
        if (TAIL && i == nq) { n_lpL = m.lpL; n_lpR = m.lpR; n_apL = m.apL; n_apR = m.apR; }
        v2f ml = xl[i], mr = xr[i];
        if (xf) {
            v2f lpl = mad2<FMA>(a0, ml, b1 * m.lpL);          // crossfeed.c:137-138
            v2f lpr = mad2<FMA>(a0, mr, b1 * m.lpR);
            m.lpL = lpl; m.lpR = lpr;
            v2f apl = mad2<FMA>(apa, lpl, m.apL);             // :145-148
            m.apL = mad2<FMA>(-apa, apl, lpl);
            v2f apr = mad2<FMA>(apa, lpr, m.apR);
            m.apR = mad2<FMA>(-apa, apr, lpr);
            v2f dl = (ml - lpl) + apr;
            v2f dr = (mr - lpr) + apl;
            ml = dl; mr = dr;
        }
        xch[i * HALF] = ml;
        xch[(T + i) * HALF] = mr;
    }
    if (TAIL && nq != T) { m.lpL = n_lpL; m.lpR = n_lpR; m.apL = n_apL; m.apR = n_apR; }
    if (cq == g.cpb - 1) {   // usb_audio.c:963-966
        // (addresses from an opaque copy of the stream index, formed once per packet: otherwise (stream + c) * n_blocks is hoisted out of
        //  the time loop as two 64-bit values per lane and lives in scratch for the whole launch.  Not in the per-lane-value variants:
        //  there the same statement moves the allocator's choices the other way: 12.1 instead of 11.1 ms with identical filters, 18.5 instead
        //  of 16.2 ms in the every-filter-differs case)
        uint32_t stream_ = stream, lane_ = lane;
        if constexpr (!PV) asm volatile("" : "+v"(stream_), "+v"(lane_));
        uint32_t *gs = a.state + (size_t)wg * sm.n_slots * ROWP + lane_ * 2;
        v2u p0, p1;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            p0[c] = (uint32_t)(fminf(1.0f, m.pk_l[c]) * 32767.0f);
            p1[c] = (uint32_t)(fminf(1.0f, m.pk_r[c]) * 32767.0f);
            if (m.pk_l[c] > 1.001f) m.clip[c] |= 1u;
            if (m.pk_r[c] > 1.001f) m.clip[c] |= 2u;
            if (a.peaks) {
                uint16_t *pp = a.peaks + ((size_t)(stream_ + c) * g.n_blocks + kq) * sm.n_ch;
                pp[0] = (uint16_t)p0[c]; pp[1] = (uint16_t)p1[c];
            }
        }
        *reinterpret_cast<v2u *>(gs + (sm.peaks + 0) * ROWP) = p0;
        *reinterpret_cast<v2u *>(gs + (sm.peaks + 1) * ROWP) = p1;
    }
}

template <bool TAIL, bool PCM24, bool FMA, bool PV, bool PVB = PV>
__device__ __forceinline__ void master_intake_pk(const KArgs &a, ImgPtr img, const float *tile, const StateMap &sm, const Geo &g, MasterPk &m,
                                                 v2f (&xl)[T], v2f (&xr)[T], v2f *__restrict__ lds_state, v2f *__restrict__ mailbox,
                                                 uint32_t *ring, uint32_t *ring_r, uint32_t lane, uint32_t stream, bool lev_on, uint32_t k1, uint32_t c1) {
    const uint32_t flags = img->flags;
    const int n = TAIL ? (int)min((uint32_t)T, g.B - c1 * T) : T;
    // ---- input conversion + preamp (usb_audio.c:591-686) ----
    const size_t frame0 = ((size_t)stream * g.n_blocks + k1) * g.B + (size_t)c1 * T;
    const size_t fstride = (size_t)g.n_blocks * g.B;        // frames between the lane's two streams
    if (PCM24) {
        const auto gl = (1.0f / 8388608.0f) * pv_val<PV>(tile, lane, PV_PREAMP0, img->preamp[0].f), gr = (1.0f / 8388608.0f) * pv_val<PV>(tile, lane, PV_PREAMP1, img->preamp[1].f);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint16_t *p = reinterpret_cast<const uint16_t *>(static_cast<const uint8_t *>(a.pcm) + (frame0 + c * fstride) * 6);
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const int j = (TAIL && i >= n) ? n - 1 : i;       // ragged chunk: re-read the last frame (stays inside the buffer)
                uint32_t w0 = p[j * 3], w1 = p[j * 3 + 1], w2 = p[j * 3 + 2];
                int32_t l = (int32_t)((w0 | (w1 << 16)) << 8) >> 8;
                int32_t r = (int32_t)(((w1 >> 8) | (w2 << 8)) << 8) >> 8;
                xl[i][c] = (float)l;
                xr[i][c] = (float)r;
            }
        }
#pragma unroll
        for (int i = 0; i < T; ++i) { xl[i] = xl[i] * gl; xr[i] = xr[i] * gr; }
    } else {
        const auto gl = (1.0f / 32768.0f) * pv_val<PV>(tile, lane, PV_PREAMP0, img->preamp[0].f), gr = (1.0f / 32768.0f) * pv_val<PV>(tile, lane, PV_PREAMP1, img->preamp[1].f);
        const uint32_t *p = static_cast<const uint32_t *>(a.pcm) + frame0;
        if (!TAIL) {
            if (!m.pre_valid) {
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int v = 0; v < T / 4; ++v) m.pre[c][v] = ld4(p + c * fstride + v * 4);
            }
            pcm16_to_f(m.pre[0], 0, xl, xr);
            pcm16_to_f(m.pre[1], 1, xl, xr);
            m.pre_valid = 0;        // the next chunk is requested at the end of the step (master_prefetch_pk)
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    uint32_t w = p[c * fstride + (i >= n ? n - 1 : i)];       // ragged chunk: re-read the last frame
                    xl[i][c] = (float)(int32_t)(int16_t)(w & 0xffffu);
                    xr[i][c] = (float)((int32_t)w >> 16);
                }
        }
#pragma unroll
        for (int i = 0; i < T; ++i) { xl[i] = xl[i] * gl; xr[i] = xr[i] * gr; }
    }
    // ---- loudness shelves (usb_audio.c:688-718) ----
    // left and right interleaved (run_bands16_pk2)
    const bool l_on = !(img->ch_bypassed & 1u), r_on = !(img->ch_bypassed & 2u);
    // (per-lane master filters never come here: with the leveller on the channels run on two waves, with it off one after the other
    //  on this wave — master_intake_pv; this function then serves the rows whose master filters are the same in every stream)
    run_bands16_pk2<2, true, TAIL, FMA>(xl, xr, img->loud, img->loud, true, true, lds_state + (sm.loud + 0) * HALF + lane,
                                   lds_state + (sm.loud + 4) * HALF + lane, (uint32_t)n);
    // ---- master EQ (usb_audio.c:721-728) ----
    if (!(flags & IF_BYPASS_MASTER_EQ) && (l_on || r_on))
        run_bands16_pk2<kBands, false, TAIL, FMA>(xl, xr, img->eq[0], img->eq[1], l_on, r_on, lds_state + (sm.eq + 0) * HALF + lane,
                                             lds_state + (sm.eq + kBands * 2) * HALF + lane, (uint32_t)n);
    if (lev_on) {
        // ---- leveller pass 1: RMS envelopes (leveller.c:155-172), samples parked in the ring ----
        const auto ar = pv_val<PV>(tile, lane, PV_LV + 0, img->lv_alpha_rms), nar = 1.0f - ar;
        v2f n_el = m.env_l, n_er = m.env_r;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (TAIL && i == n) { n_el = m.env_l; n_er = m.env_r; }
            m.env_l = mad2<FMA>(ar, m.env_l, nar * (xl[i] * xl[i]));      // leveller.c:165-166
            m.env_r = mad2<FMA>(ar, m.env_r, nar * (xr[i] * xr[i]));
        }
        if (TAIL && n != T) { m.env_l = n_el; m.env_r = n_er; }      // ragged chunk: the envelopes after n samples
        const v2u base = (m.rp1 + c1 * T) & (uint32_t)(kRingLen - 1);
        // Ring rows are read back by the hand-off wave two or more steps from now.  Draining here (everything older than
        // the EQ above has long landed, so this costs nothing) means: once the barrier that ends step s+1 has been
        // passed, the rows stored in step s are complete.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        rows_store<TAIL>(xl, n, ring, lane * 2, base, kRingLen - 1);
        rows_store<TAIL>(xr, n, ring_r, lane * 2, base, kRingLen - 1);
        if (c1 == g.cpb - 1) {   // end of packet: gain decision (leveller.c:168-206), per stream
            struct LvC { float lv_alpha_attack, lv_alpha_release, lv_threshold_db, lv_ratio, lv_knee_db, lv_makeup_db, lv_gate_db, lv_max_gain_db; };
            v2f lvv[8];
            if constexpr (PV) {
#pragma unroll
                for (int k = 0; k < 8; ++k) lvv[k] = pv_val<true>(tile, lane, PV_LV + 1 + k, 0.0f);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float el = m.env_l[c], er = m.env_r[c], gsm = m.gsm_db[c];
                if (el < 1e-30f) el = 0.0f;
                if (er < 1e-30f) er = 0.0f;
                float rms_sq = (el > er) ? el : er;
                float gn;
                if constexpr (PV) {
                    const LvC lvc{lvv[0][c], lvv[1][c], lvv[2][c], lvv[3][c], lvv[4][c], lvv[5][c], lvv[6][c], lvv[7][c]};
                    gn = leveller_block_gain<FMA>(&lvc, gsm, rms_sq, g.B);
                } else gn = leveller_block_gain<FMA>(img, gsm, rms_sq, g.B);
                m.env_l[c] = el; m.env_r[c] = er; m.gsm_db[c] = gsm;
                m.g_prev[c] = m.g_cur[c];
                m.g_cur[c] = gn;
            }
            mailbox[(k1 & (kMailbox - 1)) * HALF + lane] = m.g_cur;
            m.rp1 = (m.rp1 + g.B) & (uint32_t)(kRingLen - 1);
        }
    }
}

// per-packet gain decision with per-lane leveller numbers (leveller.c:174-206); env_l / m.env_r are the flushed end-of-packet envelopes
template <bool FMA>
__device__ __forceinline__ void pv_gain_decision(const float *tile, uint32_t lane, MasterPk &m, v2f env_l, uint32_t B, v2f *__restrict__ mailbox, uint32_t k) {
    struct LvC { float lv_alpha_attack, lv_alpha_release, lv_threshold_db, lv_ratio, lv_knee_db, lv_makeup_db, lv_gate_db, lv_max_gain_db; };
    v2f lvv[8];
    asm volatile("" : "+v"(lane));      // (tile offsets formed here, see master_handoff_pk)
#pragma unroll
    for (int j = 0; j < 8; ++j) lvv[j] = pv_val<true>(tile, lane, PV_LV + 1 + j, 0.0f);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float el = env_l[c], er = m.env_r[c];
        float gsm = m.gsm_db[c];
        const float rms_sq = (el > er) ? el : er;
        const LvC lvc{lvv[0][c], lvv[1][c], lvv[2][c], lvv[3][c], lvv[4][c], lvv[5][c], lvv[6][c], lvv[7][c]};
        const float gn = leveller_block_gain<FMA>(&lvc, gsm, rms_sq, B);
        m.gsm_db[c] = gsm;
        m.g_prev[c] = m.g_cur[c];
        m.g_cur[c] = gn;
    }
    mailbox[(k & (kMailbox - 1)) * HALF + lane] = m.g_cur;
}

// Per-lane values, leveller on: the two channels go through the wave ONE AFTER THE OTHER on a single sample array — with the
// leveller on every sample is parked in the ring anyway, so nothing needs left and right at the same time, and the 32 registers
// of the second array pay for the coefficient pairs and their look-ahead (run_bands16_pkv).  16-bit input words are read twice
// (the second time from this CU's L1).  Same arithmetic, same order per channel as master_intake_pk.
// `side`: 0 = both channels in this wave, which also takes the packet's gain decision; 1 / 2 = the LEFT / RIGHT channel only (the
// three waves of the master SIMD share the work: the intake wave takes the left channel, the third wave — the copy wave of the
// stream-major layout, idle otherwise — the right one, each posts its end-of-packet envelope in LDS, and the hand-off wave takes the
// decision at the start of the next step — see the kernel body).
template <bool TAIL, bool PCM24, bool FMA>
__device__ __forceinline__ void master_intake_pv(const KArgs &a, ImgPtr img, const float *tile, const StateMap &sm, const Geo &g, MasterPk &m,
                                                 v2f (&x)[T], v2f *__restrict__ lds_state, v2f *__restrict__ mailbox, v2f *__restrict__ envpost,
                                                 uint32_t *ring, uint32_t *ring_r, uint32_t lane, uint32_t stream, uint32_t k1, uint32_t c1, int side = 0,
                                                 v2f *__restrict__ park = nullptr) {
    // park != nullptr: leveller OFF (side 0).  No envelopes, no ring: each channel's chunk is parked in LDS — the slots of this chunk's
    // crossfeed output, [2][T][64], which the hand-off of the same step reads back and then overwrites.  (Both channels band by band on
    // two sample arrays, as the shared-coefficient loops do it, spilled one array per band: 32 scratch instructions per band visit.)
    const uint32_t flags = img->flags;
    const int n = TAIL ? (int)min((uint32_t)T, g.B - c1 * T) : T;
    const size_t frame0 = ((size_t)stream * g.n_blocks + k1) * g.B + (size_t)c1 * T;
    const size_t fstride = (size_t)g.n_blocks * g.B;
    const v2f ar = pv_val<true>(tile, lane, PV_LV + 0, 0.0f), nar = 1.0f - ar;
    const v2u base = (m.rp1 + c1 * T) & (uint32_t)(kRingLen - 1);
#pragma unroll 1
    for (int ch = (side == 2 ? 1 : 0); ch < (side == 1 ? 1 : 2); ++ch) {
        const v2f pre = pv_val<true>(tile, lane, PV_PREAMP0 + ch, 0.0f);
        if (PCM24) {
            const v2f gsc = (1.0f / 8388608.0f) * pre;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint16_t *p = reinterpret_cast<const uint16_t *>(static_cast<const uint8_t *>(a.pcm) + (frame0 + c * fstride) * 6);
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const int j = (TAIL && i >= n) ? n - 1 : i;
                    const uint32_t w0 = p[j * 3], w1 = p[j * 3 + 1], w2 = p[j * 3 + 2];
                    const int32_t l = (int32_t)((w0 | (w1 << 16)) << 8) >> 8;
                    const int32_t r = (int32_t)(((w1 >> 8) | (w2 << 8)) << 8) >> 8;
                    x[i][c] = (float)(ch ? r : l);
                }
            }
#pragma unroll
            for (int i = 0; i < T; ++i) x[i] = x[i] * gsc;
        } else {
            const v2f gsc = (1.0f / 32768.0f) * pre;
            const uint32_t *p = static_cast<const uint32_t *>(a.pcm) + frame0;
            if (!TAIL) {      // whole chunks: four 16-byte loads per stream (a 4-byte load per frame is 64 cache lines per instruction, 32 instructions)
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    u32x4 w[T / 4];
#pragma unroll
                    for (int v = 0; v < T / 4; ++v) w[v] = ld4(p + c * fstride + v * 4);
#pragma unroll
                    for (int v = 0; v < T / 4; ++v)
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[v * 4 + e][c] = ch ? (float)((int32_t)w[v][e] >> 16) : (float)(int32_t)(int16_t)(w[v][e] & 0xffffu);
                }
            } else
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const uint32_t w = p[c * fstride + ((TAIL && i >= n) ? n - 1 : i)];
                    x[i][c] = ch ? (float)((int32_t)w >> 16) : (float)(int32_t)(int16_t)(w & 0xffffu);
                }
#pragma unroll
            for (int i = 0; i < T; ++i) x[i] = x[i] * gsc;
        }
        run_bands16_pkv<2, FMA, TAIL>(x, img->loud, true, tile, kMaxCh * kBands, lane, lds_state + (sm.loud + 4 * ch) * HALF + lane, (uint32_t)n);
        if (!(flags & IF_BYPASS_MASTER_EQ) && !((img->ch_bypassed >> ch) & 1u))
            run_bands16_pkv<kBands, FMA, TAIL>(x, img->eq[ch], true, tile, ch * kBands, lane, lds_state + (sm.eq + ch * kBands * 2) * HALF + lane, (uint32_t)n);
        if (park) {
#pragma unroll
            for (int i = 0; i < T; ++i) park[(ch * T + i) * HALF] = x[i];
            continue;
        }
        v2f env = ch ? m.env_r : m.env_l, n_e = env;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            if (TAIL && i == n) n_e = env;
            env = mad2<FMA>(ar, env, nar * (x[i] * x[i]));      // leveller.c:165-166
        }
        if (TAIL && n != T) env = n_e;
        if (ch) m.env_r = env; else m.env_l = env;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // see master_intake_pk
        rows_store<TAIL>(x, n, ch ? ring_r : ring, lane * 2, base, kRingLen - 1);
    }
    if (!park && c1 == g.cpb - 1) {   // end of packet
        // the envelopes are flushed where they would be denormal (leveller.c:168-173), each by the wave that carries it
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (side != 2 && m.env_l[c] < 1e-30f) m.env_l[c] = 0.0f;
            if (side != 1 && m.env_r[c] < 1e-30f) m.env_r[c] = 0.0f;
        }
        if (side == 0) pv_gain_decision<FMA>(tile, lane, m, m.env_l, g.B, mailbox, k1);
        if (side == 1) envpost[(k1 & 1u) * HALF + lane] = m.env_l;
        if (side == 2) envpost[(2 + (k1 & 1u)) * HALF + lane] = m.env_r;
        m.rp1 = (m.rp1 + g.B) & (uint32_t)(kRingLen - 1);
    }
}

// Next chunk's input words, requested at the END of the intake wave's step: the two interleaved EQ channels need the
// registers a whole-step-ahead request would occupy, and the intake wave now reaches the barrier well before the output
// waves, so the latency falls into that wait.  (16-bit input, full chunks; chunks of one stream are contiguous across packets.)
template <bool TAIL, bool PCM24>
__device__ __forceinline__ void master_prefetch_pk(const KArgs &a, const Geo &g, MasterPk &m, uint32_t stream, uint32_t k1, uint32_t c1) {
    if (TAIL || PCM24) return;
    const bool more = (c1 + 1 < g.cpb) || (k1 + 1 < g.n_blocks);
    m.pre_valid = more;
    if (!more) return;
    const size_t frame0 = ((size_t)stream * g.n_blocks + k1) * g.B + (size_t)c1 * T;
    const size_t fstride = (size_t)g.n_blocks * g.B;
    const uint32_t *p = static_cast<const uint32_t *>(a.pcm) + frame0;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int v = 0; v < T / 4; ++v) m.pre[c][v] = ld4(p + c * fstride + T + v * 4);
}

// ring rows of chunk (kq, cq) for pass 2: the lookahead line is the same ring read kLookahead samples back
template <bool TAIL>
__device__ __forceinline__ void master_fetch_pk(ImgPtr img, const Geo &g, const MasterPk &m, v2f (&xl)[T], v2f (&xr)[T],
                                                const uint32_t *ring, const uint32_t *ring_r, uint32_t lane, uint32_t cq) {
    const int nq = TAIL ? (int)min((uint32_t)T, g.B - cq * T) : T;
    const uint32_t back = (img->flags & IF_LOOKAHEAD) ? (uint32_t)kLookahead : 0u;
    const v2u base = (m.rp2 + (cq * T - back)) & (uint32_t)(kRingLen - 1);
    rows_load<TAIL, true>(xl, nq, ring, lane * 2, base, kRingLen - 1);
    rows_load<TAIL, true>(xr, nq, ring_r, lane * 2, base, kRingLen - 1);
}

// ==========================================================================================
// output waves
// ==========================================================================================
struct OutPk {
    v2u widx;
    v2u loading, counter;
    v2f smooth;
    v2f vmm;
    v2u clip;
    // A wave either emits its pair's stream-major words (a pair output on the stream-major layout) or writes its own words ahead (every
    // output of the tiled layout, the sub): the two sets of meters share their registers.
    //   pair emission:  u_pk[0], u_pk[1] = running packet peaks of the pair's two outputs over this wave's half of the frames;
    //                   u_w = this wave's own output, the packet just ended: its half's meter word until the partner's half arrives
    //   words ahead:    u_pk[0] = running peak of the packet the ahead stream is in, u_pk[1] = the ahead part of the packet that also takes
    //                   frames from the line at the launch's head; u_w = the packet the ahead stream is in
    v2f u_pk[2];
    uint32_t u_w;
};

// launch-invariant parameters of the wave's output, read from the image once before the time loop (re-reading them
// every step puts a scalar-load round trip at the head of each step)
template <bool PV>
struct OutConst {
    uint32_t flags;
    bool enabled, muted, ch_bypassed;
    bool gl_nz, gr_nz;     // the crosspoint's zero pattern (structure: the same for every stream of a PV row)
    bool bands_differ;     // per-lane filters: some band of this output differs between the row's streams (else: the image's scalars)
    int32_t dly;
    typename PvT<PV>::type gl, gr, og;
    float word_scale;      // 8388607, or 0 for a pair whose two outputs are both disabled: zero-filled whatever its delay
                           // lines still hold (usb_audio.c:930-933)
    uint32_t dly_k, dly_r; // dly / B and dly % B: the packet in which the words written ahead begin, and where in it
};
template <bool PV>
__device__ __forceinline__ OutConst<PV> load_out_const(ImgPtr img, const float *tile, uint32_t lane, int o, uint32_t B) {
    OutConst<PV> k;
    k.flags = img->flags;
    k.enabled = (img->out_enabled >> o) & 1u;
    k.word_scale = (((img->out_enabled >> o) | (img->out_enabled >> (o ^ 1))) & 1u) ? 8388607.0f : 0.0f;
    k.muted = (img->out_mute >> o) & 1u;
    k.ch_bypassed = (img->ch_bypassed >> (2 + o)) & 1u;
    k.dly = img->delay_samples[o];
    k.dly_k = (uint32_t)k.dly / B; k.dly_r = (uint32_t)k.dly % B;
    k.gl_nz = img->mix[0][o].f != 0.0f; k.gr_nz = img->mix[1][o].f != 0.0f;
    k.bands_differ = PV && tile && pv_differ(tile, (2 + o) * kBands, kBands) != 0u;
    k.gl = pv_val<PV>(tile, lane, PV_MIX0 + o, img->mix[0][o].f); k.gr = pv_val<PV>(tile, lane, PV_MIX1 + o, img->mix[1][o].f);
    k.og = pv_val<PV>(tile, lane, PV_OG + o, img->out_gain_lin[o]);
    return k;
}

// H rows of a [position][128] array written by ANOTHER wave (agent-scope loads, see rows_load) into d[OFF .. OFF + H)
constexpr int H = T / 2;
template <int OFF>
__device__ __forceinline__ void rows_load_half(v2f (&d)[T], const uint32_t *base, uint32_t lo, v2u p, uint32_t pmask) {
    if (DSPI_EXP_EMIT & 2) {
#pragma unroll
        for (int i = 0; i < H; ++i) d[OFF + i] = splat(0.25f);
    } else if (__all(p.x == p.y && p.x + H <= pmask + 1u)) {
        const uint32_t off = p.x * ROWP + lo;
#pragma unroll
        for (int i = 0; i < H; ++i) d[OFF + i] = as_v2f(ld_agent2(base + (off + i * ROWP)));
    } else {
        uint32_t px = p.x, py = p.y;
        asm volatile("" : "+v"(px), "+v"(py));
#pragma unroll
        for (int i = 0; i < H; ++i) {
            d[OFF + i].x = as_f(ld_agent(base + (((px + i) & pmask) * ROWP + lo)));
            d[OFF + i].y = as_f(ld_agent(base + (((py + i) & pmask) * ROWP + lo + 1)));
        }
    }
}
// a packet's meter of one output as it travels between the two waves of a pair and into the status: per stream 15 bits of peak
// (min(1, p) * 32767, usb_audio.c:915-923) and the clip bit (p > 1.001); the conversion is monotonic, so the maximum of two halves' words
// is the word of the maximum
__device__ __forceinline__ uint32_t meter_word(v2f pk) {
    uint32_t w = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) w |= (((uint32_t)(fminf(1.0f, pk[c]) * 32767.0f)) | (pk[c] > 1.001f ? 0x8000u : 0u)) << (16 * c);
    return w;
}
__device__ __forceinline__ uint32_t meter_max(uint32_t a, uint32_t b) {      // per 16-bit half: max of the peaks, OR of the clip bits
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint32_t x = (a >> (16 * c)) & 0xffffu, y = (b >> (16 * c)) & 0xffffu;
        r |= (max(x & 0x7fffu, y & 0x7fffu) | ((x | y) & 0x8000u)) << (16 * c);
    }
    return r;
}

// One step of an output wave: chunk q = (kq, cq) of output o.
//
// Stream-major words (!TILED; the firmware's own layout: one interleaved L/R buffer per stream and S/PDIF pair, usb_audio.c:934-940).  What those
// buffers hold are DELAYED samples of TWO outputs, and the two outputs are computed by two waves.  Round 2 had each wave convert its words
// into an exchange area in HBM and a copy wave gather them into whole lines (72 B/frame of exchange traffic next to the delay lines' 64;
// writing them directly scatters 4-byte words: 64 cache lines per store instruction, 1.7x slower).  Now the delay line itself is the
// hand-over — it already is the place where a sample waits for its frame:
//   * a wave stores its chunk's rows into its output's line (what the reference's line[w] = x costs anyway) and emits nothing of its own;
//   * two chunks later BOTH waves of a pair read the rows of frame f - dly of BOTH sides, each for HALF of the chunk's frames (wave 2p: the
//     first eight, wave 2p + 1: the last eight; whole 8-byte rows, every row read once), requested before the EQ and landing under it like
//     the tiled layout's delayed rows;
//   * after the EQ each converts its frames of both streams (clamp, scale, truncate: usb_audio.c:926-941) and writes half a line (64 bytes,
//     four 16-byte stores) of [stream][pair][frame][2] per stream — the two waves together one whole 128-byte line per stream and chunk;
//   * the meters (:915-923): each wave keeps the running packet peak of BOTH outputs over its half of the frames; at a packet's end it posts
//     its half's word for the partner's output in LDS (meter_word, double-buffered by packet parity) and, one step later, finishes its OWN
//     output's packet from its own half and the partner's.
// Per sample and output the chain moves 12 bytes (line store, line load, word) instead of 20, there is no copy wave, and an output wave
// issues 48 row accesses and 8 line stores per step instead of 32 and 8 (+ the copy wave's 72 loads and 36 stores per workgroup).
// An output whose line the reference does not write (delay 0) or whose delayed rows the partner's NEXT chunk of stores could overwrite
// before they are read (delays within three chunks of the line's length: the rows just ahead of the write index) hands its rows over
// through a three-chunk mini line in a.xwords instead; for the latter the wave reads its line first, in the reference's order.
// The sub (no partner) emits its own words as on the tiled layout.  `work` false: only the emission of the launch's last chunk is left.
template <bool TAIL, bool TILED, bool FMA, bool PV, bool PVB = PV>
__device__ __forceinline__ void output_item_pk(const KArgs &a, ImgPtr img, const float *tile, const OutConst<PV> &oc, const StateMap &sm, const Geo &g, OutPk &s,
                                               v2f *__restrict__ lds_state, v2f *__restrict__ lds_pk, const v2f *__restrict__ xch_base,
                                               uint32_t wg, uint32_t lane, uint32_t stream, int o,
                                               uint32_t kq, uint32_t cq, uint32_t q, bool work = true, bool emit_prev = false, uint32_t e_kq = 0, uint32_t e_cq = 0,
                                               bool fin_prev = false, uint32_t fin_k = 0) {
    const uint32_t flags = oc.flags;
    [[maybe_unused]] const unsigned long long wt_in = WT_NOW();
    const int n = TAIL ? (int)min((uint32_t)T, g.B - cq * T) : T;
    constexpr int N = make_state_map(1).n_out, P = make_state_map(1).n_pairs;
    const bool is_sub = (o == N - 1);
    const bool sm_pair = !TILED && !is_sub;      // this wave emits one stream of its pair, a chunk late
    const size_t F = (size_t)g.n_blocks * g.B;
    const uint32_t dmask = (uint32_t)sm.max_delay - 1u;
    const bool sub_active = flags & IF_SUB_ACTIVE;
    const int eh = o & 1;                        // the half of a chunk's frames this wave emits
    // where the emit side finds the rows of output `oo`: its delay line at frame - dly, or the mini line
    auto e_direct = [&](int oo, int32_t dly_) {
        const bool dl_on_ = (flags & IF_ANY_DELAY) && dly_ > 0;      // (pair outputs are always processed)
        return dl_on_ && (dly_ >= sm.max_delay || dly_ <= sm.max_delay - 3 * T);
    };
    // ---- (stream-major pairs) the delayed rows of both sides for this wave's half of the chunk to emit: requested now, landing under the EQ ----
    v2f dl[T];      // stream-major pairs: [0, 8) left side, [8, 16) right side of this wave's eight frames; else: this output's delayed rows
    // the chunk to emit is q - 2 = (e_kq, e_cq): the rows of step st are drained in the middle of step st + 1 (below), so they are complete
    // behind the barrier that ends step st + 1 — the intake wave's scheme for the leveller ring — and no wave waits for its stores
    const uint32_t e_q = q - 2u;
    // (the write index as of the chunk to emit: it advances by a packet's frames at every packet's end while a delay is active, usb_audio.c:911)
    const v2u e_w0 = s.widx - ((flags & IF_ANY_DELAY) ? (kq - e_kq) * g.B : 0u) + (e_cq * T + (uint32_t)eh * H);
    uint32_t *mail = reinterpret_cast<uint32_t *>(lds_pk + 2 * HALF);      // [2 parities][8 pair outputs][64 lanes] meter words (the slots of the tiled layout's running peaks)
    if (fin_prev) {      // the packet that ended with the chunk emitted a step ago: this wave's own output, both halves of the frames
        const uint32_t wd = meter_max(s.u_w, mail[((fin_k & 1u) * 8u + (uint32_t)o) * 64u + lane]);
        uint32_t stream_ = stream, lane_ = lane;
        asm volatile("" : "+v"(stream_), "+v"(lane_));
        v2u p16;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            p16[c] = (wd >> (16 * c)) & 0x7fffu;
            if ((wd >> (16 * c)) & 0x8000u) s.clip[c] |= 1u << (2 + o);
            if (a.peaks) a.peaks[((size_t)(stream_ + c) * g.n_blocks + fin_k) * sm.n_ch + 2 + o] = (uint16_t)p16[c];
        }
        if (fin_k == g.n_blocks - 1) *reinterpret_cast<v2u *>(a.state + ((size_t)wg * sm.n_slots + sm.peaks + 2 + o) * ROWP + lane_ * 2) = p16;
    }
    if (emit_prev) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int oo = (o & ~1) + side;
            const int32_t dly_ = img->delay_samples[oo];
            const bool direct_ = e_direct(oo, dly_);
            const uint32_t *src = direct_ ? a.dlines + ((size_t)wg * N + oo) * (size_t)sm.max_delay * ROWP
                                          : a.xwords + (((size_t)wg * 3 + (e_q % 3u)) * kMaxOut + oo) * (T * ROWP);
            const v2u pos = direct_ ? ((e_w0 - (uint32_t)dly_) & dmask) : v2u{(uint32_t)eh * H, (uint32_t)eh * H};
            const uint32_t pm = direct_ ? dmask : (uint32_t)T - 1u;
            if (side) rows_load_half<H>(dl, src, lane * 2, pos, pm); else rows_load_half<0>(dl, src, lane * 2, pos, pm);
        }
    }
    if (work) {
    if (cq == 0) {
        // ---- packet scalars, per stream: preset-mute envelope (usb_audio.c:466-498) and volumes (:564-571) ----
        float step = (float)g.B / (float)img->mute_transition;
        if (step > 1.0f) step = 1.0f;
        const auto vol_ = pv_val<PV>(tile, lane, PV_VOL, img->vol.f), master_ = pv_val<PV>(tile, lane, PV_MASTER, img->master.f);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bool act = s.loading[c] != 0;
            if (act) {
                if (s.counter[c] > g.B) s.counter[c] -= g.B;
                else { s.counter[c] = 0; s.loading[c] = 0; }
            }
            float target = act ? 0.0f : 1.0f;
            float gg = s.smooth[c];
            if (gg < target) { gg += step; if (gg > target) gg = target; }
            else if (gg > target) { gg -= step; if (gg < target) gg = target; }
            s.smooth[c] = gg;
            float vol_mul = pv_c(vol_, c);
            vol_mul *= gg;
            s.vmm[c] = vol_mul * pv_c(master_, c);
        }
    }
    // post-crossfeed L/R chunk: re-read from LDS for every output (LDS reads are free next to the VALU work; holding
    // 2 x 32 registers across the band loops is not)
    const v2f *xch = xch_base + (size_t)(q & 1u) * (2 * T * HALF) + lane;
    const size_t frame0 = (size_t)kq * g.B + (size_t)cq * T;
    {   // one output per wave
        [[maybe_unused]] const unsigned long long wt0 = WT_NOW();
#ifdef DSPI_WT_TOP
        WT_PHASE(3 + o, 1, wt0 - wt_in);      // (development: the top of the step — finishing a packet's meters, requesting the rows to emit, packet scalars — instead of the drain)
#endif
        const bool processed = !is_sub || sub_active;
        const bool enabled = oc.enabled;
        const bool muted = oc.muted;
        v2f x[T];
        const int32_t dly = oc.dly;
        const bool dl_on = processed && (flags & IF_ANY_DELAY) && dly > 0;
        const bool dl_alias = dl_on && dly >= sm.max_delay;
        const bool dl_early = dl_on && !dl_alias && dly >= T;
        uint32_t *line = a.dlines + ((size_t)wg * N + o) * (size_t)sm.max_delay * ROWP;      // wave-uniform
        const v2u w0 = s.widx + cq * T;
        const v2u wb = w0 & dmask, rb = (w0 - (uint32_t)dly) & dmask;
        const bool xdirect = sm_pair && dl_on && (dl_alias || dly <= sm.max_delay - 3 * T);
        const bool xhazard = sm_pair && dl_on && !xdirect;
        uint32_t *mini = sm_pair ? a.xwords + (((size_t)wg * 3 + (q % 3u)) * kMaxOut + o) * (T * ROWP) : nullptr;      // wave-uniform
        // delayed samples: requested now, landing under the EQ below (requesting them a whole step ahead was tried and
        // lost more to the loop-carried register array than it won)
        // Words written AHEAD (every output of the tiled layout, the sub on either layout; SURVEY.md 8d's launch-span accounting).  The delay
        // is a pure shift (usb_audio.c:898-912: line[w] = x; x = line[w - dly]) and nothing after it depends on the packet (word scale,
        // enables and the I2S shift are the launch's), so the word of frame f + dly is known at frame f: it is converted and stored THEN,
        // straight to its future frame, and the sample goes through the line only where the launch ends first — the launch's last frames,
        // which the next launch reads back at its head (frames < dly).  What the line must hold is what the reference's holds: the last
        // max_delay samples (a later, LONGER delay reads further back, and neither REQ_SET_DELAY nor a bulk load clears the lines:
        // usb_audio.c:1683-1692, main.c:1126-1162), so the launch's last min(F, max_delay) frames are stored, whatever the delay.
        // Per frame: 4 B of word, + 4 B of line store for the launch's last max_delay frames, + 4 B of line load for its first dly
        // (was: 4 + 4 + 4 always).  The meters follow the words: a packet's peak is the maximum over the frames taken from the line (head)
        // and over the frames written ahead, which cross a packet boundary at most once per chunk.
        const bool ahead = !sm_pair && dl_on && !dl_alias && (size_t)dly < F;
        const bool head = ahead && frame0 < (size_t)dly;                       // this chunk still has frames that come from the line
        const size_t hist = F < (size_t)sm.max_delay ? F : (size_t)sm.max_delay;
        const bool keep = frame0 + T > F - hist;                               // this chunk lies (partly) in the launch's last max_delay frames
        if (!sm_pair && (ahead ? head : dl_early)) rows_load<TAIL>(dl, n, line, lane * 2, rb, dmask);
        if (xhazard) {
            // the delayed rows lie just ahead of the write index: read BEFORE this chunk's stores overwrite them (the reference's order, sample
            // by sample: usb_audio.c:905-907) and handed on through the mini line at once (a rare delay: the wait is exposed; x is not live yet)
            rows_load<TAIL>(x, n, line, lane * 2, rb, dmask);
            rows_store<TAIL>(x, n, mini, lane * 2, v2u{0u, 0u}, (uint32_t)T - 1u);
        }
        // ---- matrix mix (usb_audio.c:753-779) ----
        const auto gl = here(oc.gl), gr = here(oc.gr);
        // One multiply from the first contributing input, the second term added in place, the all-zero case overwritten in
        // place: every variant updates the SAME registers, so the uniform branches do not turn into register shuffles.
        // (firmware contract: buf_l*gl + buf_r*gr is fma(buf_l, gl, buf_r*gr) — the right product is the rounded one, so
        //  it goes first and the left one is fused onto it)
        {
            const bool first_l = FMA ? !oc.gr_nz : oc.gl_nz;
            const v2f *src = xch + (first_l ? 0 : T * HALF);
            const auto g1 = first_l ? gl : gr;
#pragma unroll
            for (int i = 0; i < T; ++i) x[i] = src[i * HALF] * g1;
            if (enabled && oc.gl_nz && oc.gr_nz) {
#pragma unroll
                for (int i = 0; i < T; ++i) x[i] = FMA ? mad2<true>(gl, xch[i * HALF], x[i]) : x[i] + xch[(T + i) * HALF] * gr;
            }
            if (!enabled || (!oc.gl_nz && !oc.gr_nz)) {
#pragma unroll
                for (int i = 0; i < T; ++i) x[i] = splat(0.0f);
            }
        }
        if (processed) {
            // ---- per-output EQ + gain (usb_audio.c:877-895) ----
            if (enabled) {
                const int ch = 2 + o;
                if (!muted && !oc.ch_bypassed) {
                    if (PVB && oc.bands_differ) {
                        if constexpr (PVB) run_bands16_pkv<kBands, FMA, TAIL>(x, img->eq[ch], true, tile, ch * kBands, lane, lds_state + (sm.eq + ch * kBands * 2) * HALF + lane, (uint32_t)n);
                    } else run_bands_pk<TAIL, kBands, FMA>(x, n, img->eq[ch], lds_state + (sm.eq + ch * kBands * 2) * HALF + lane);
                }
                const auto og = oc.og;
                v2f gain = muted ? splat(0.0f) : og * s.vmm;
                // in place; the reference's memset branch (gain == 0 gives +0.0, not x*0) patches the same registers
#pragma unroll
                for (int i = 0; i < T; ++i) x[i] = x[i] * gain;
                if (__any(gain.x == 0.0f || gain.y == 0.0f)) {
#pragma unroll
                    for (int i = 0; i < T; ++i) {
                        if (gain.x == 0.0f) x[i].x = 0.0f;
                        if (gain.y == 0.0f) x[i].y = 0.0f;
                    }
                }
            }
            WT_PHASE(3 + o, 0, WT_NOW() - wt0);      // mix + EQ + gain
            // ---- delay line (usb_audio.c:898-912) ----
            // (the stores are issued AFTER the output words below when the delayed samples were fetched early: nothing
            // then waits behind them, a wait for `dl` placed after the stores would drain those too)
            if (sm_pair) {
                // below: the rows go to the line or to the mini line
            } else if (dl_alias) {
                if (keep) rows_store<TAIL>(x, n, line, lane * 2, wb, dmask);      // dly == max_delay reads back what it just wrote: the line only keeps the history
            } else if (dl_on && !dl_early && !ahead) {      // delay shorter than a chunk (and a launch shorter than the delay): the reference's per-sample order
                v2u ws = w0;
                asm volatile("" : "+v"(ws));
#pragma unroll
                for (int i = 0; i < T; ++i) {       // (ragged chunk: the rows written past n lie ahead of the write index and are
                                                    //  rewritten by the next packet before anything reads them)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        uint32_t w = (ws[c] + i) & dmask;
                        line[w * ROWP + lane * 2 + c] = as_u(x[i][c]);
                        x[i][c] = as_f(line[((w - (uint32_t)dly) & dmask) * ROWP + lane * 2 + c]);
                    }
                }
            }
        }
        // ---- peaks, output words (usb_audio.c:914-959): the tiled layout's outputs, and the sub on either layout ----
        // per-stream destination addresses are formed here, once per chunk, from an opaque copy of the stream index:
        // otherwise their 64-bit bases are hoisted out of the time loop and sit in (or spill from) VGPRs for the whole launch
        uint32_t stream_ = stream, lo2 = lane * 2;
        asm volatile("" : "+v"(stream_), "+v"(lo2));
        const bool metered = !is_sub || (sub_active && enabled);
        // block maximum over rows [lo, hi) of the chunk
        auto acc_pk = [&](v2f pk, const v2f (&y)[T], int lo, int hi) {
            if (!metered) return pk;
            if (lo <= 0 && hi >= T) {
#pragma unroll
                for (int i = 0; i < T; i += 2) { pk.x = peak_acc2(pk.x, y[i].x, y[i + 1].x); pk.y = peak_acc2(pk.y, y[i].y, y[i + 1].y); }
            } else {
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const v2f v = (i >= lo && i < hi) ? y[i] : splat(0.0f);
                    pk.x = peak_acc(pk.x, v.x); pk.y = peak_acc(pk.y, v.y);
                }
            }
            return pk;
        };
        // a packet's meter is complete: peaks, sticky bit, and the status slot for the launch's last packet (usb_audio.c:915-923, :945-951)
        auto finish_packet = [&](uint32_t k, v2f pk) {
            v2u p16;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                p16[c] = metered ? (uint32_t)(fminf(1.0f, pk[c]) * 32767.0f) : 0u;
                if (metered && pk[c] > 1.001f) s.clip[c] |= 1u << (2 + o);
                if (a.peaks) a.peaks[((size_t)(stream_ + c) * g.n_blocks + k) * sm.n_ch + 2 + o] = (uint16_t)p16[c];
            }
            if (k == g.n_blocks - 1) *reinterpret_cast<v2u *>(a.state + ((size_t)wg * sm.n_slots + sm.peaks + 2 + o) * ROWP + lane * 2) = p16;
        };
        // Words of rows [0, hi) to frames dframe + i.  Tiled layout (DSPI_OUT_TILED): [tile][output][frame][128] — the wave writes one 512-byte
        // row per frame, like a delay line.  Stream-major sub: [stream][frame], 64 contiguous bytes per stream and chunk.
        auto put_words = [&](const v2f (&y)[T], size_t dframe, int hi) {
            if (hi <= 0) return;
            v2u w[T];
            if (is_sub) {
                if (!a.sub) return;
                const bool live = sub_active && enabled;
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    const v2f z = y[i] * 268435456.0f;
                    w[i] = live ? v2u{(uint32_t)f2i_sat(z.x), (uint32_t)f2i_sat(z.y)} : v2u{0u, 0u};
                }
                if (TILED) {
                    uint32_t *dst = reinterpret_cast<uint32_t *>(a.sub) + ((size_t)wg * F + dframe) * ROWP + lo2;      // one 64-bit add, rows by immediate offset
#pragma unroll
                    for (int i = 0; i < T; ++i) {
                        if (i >= hi) continue;
                        __builtin_nontemporal_store(w[i], reinterpret_cast<v2u *>(dst + i * ROWP));
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        int32_t *dst = a.sub + (size_t)(stream_ + c) * F + dframe;
                        if (hi >= T) {
#pragma unroll
                            for (int v = 0; v < T / 4; ++v) st4(dst + v * 4, u32x4{w[v * 4][c], w[v * 4 + 1][c], w[v * 4 + 2][c], w[v * 4 + 3][c]});
                        } else {
#pragma unroll
                            for (int i = 0; i < T; ++i) { if (i < hi) dst[i] = (int32_t)w[i][c]; }
                        }
                    }
                }
            } else if constexpr (TILED) {
                if (!a.pairs) return;
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    v2f d;
                    d.x = clamp_pm1(y[i].x);
                    d.y = clamp_pm1(y[i].y);
                    d = d * oc.word_scale;
                    w[i].x = (uint32_t)(int32_t)d.x;
                    w[i].y = (uint32_t)(int32_t)d.y;
                }
                if (a.i2s_slots && ((img->i2s_pairs >> (o >> 1)) & 1u)) {      // an I2S slot's words leave left-justified (audio_i2s_multi.c:217-226)
#pragma unroll                                                          // (shifting always, by 0 or 8, costs the per-lane-value kernel 10 %: 112 B/lane of scratch)
                    for (int i = 0; i < T; ++i) w[i] = w[i] << 8u;
                }
                uint32_t *dst = reinterpret_cast<uint32_t *>(a.pairs) + (((size_t)wg * (N - 1) + o) * F + dframe) * ROWP + lo2;
#pragma unroll
                for (int i = 0; i < T; ++i) {
                    if (i >= hi) continue;
                    __builtin_nontemporal_store(w[i], reinterpret_cast<v2u *>(dst + i * ROWP));      // (written once, read by nobody here)
                }
            }
        };
        // the chunk's own frames: meter in LDS across the packet's chunks, words at the chunk's frames
        auto emit = [&](const v2f (&y)[T]) {
            v2f *pkp = lds_pk + (2 + o) * HALF + lane;
            v2f pk = (cq == 0) ? splat(0.0f) : *pkp;
            pk = acc_pk(pk, y, 0, n);
            *pkp = pk;
            if (cq == g.cpb - 1) finish_packet(kq, pk);
            put_words(y, frame0, n);
        };
        [[maybe_unused]] const unsigned long long wt1 = WT_NOW();
        if (sm_pair) {
            // the previous step's rows: stored a whole EQ ago, so this wait is not one — and the barrier at the end of THIS step then
            // publishes them (the delayed rows requested at the top of this step have long arrived too)
            if (DSPI_EXP_EMIT & 16) {} else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifndef DSPI_WT_TOP
            WT_PHASE(3 + o, 1, WT_NOW() - wt1);       // (timing build) the drain
#endif
            [[maybe_unused]] const unsigned long long wt2 = WT_NOW();
            if (xdirect || xhazard) rows_store<TAIL>(x, n, line, lane * 2, wb, dmask);
            else rows_store<TAIL>(x, n, mini, lane * 2, v2u{0u, 0u}, (uint32_t)T - 1u);
            WT_PHASE(3 + o, 2, WT_NOW() - wt2);       // row stores
        } else if (ahead) {
            // (1) the frames written ahead: x[i] is the word of frame frame0 + i + dly, while that lies inside the launch
            const size_t a0 = frame0 + (size_t)dly;
            const int n_a = a0 >= F ? 0 : (int)(F - a0 < (size_t)n ? F - a0 : (size_t)n);
            if (n_a > 0) {
                auto close = [&](v2f pk) {      // the ahead stream leaves packet a_k
                    if (s.u_w == oc.dly_k && oc.dly_r != 0u) s.u_pk[1] = pk;      // (its first frames come from the line: finished at the head, below)
                    else finish_packet(s.u_w, pk);
                    s.u_w++;
                };
                const int ib = (int)((size_t)(s.u_w + 1u) * g.B - a0);      // frames left in the ahead stream's packet (>= 1)
                if (ib >= n_a) {
                    s.u_pk[0] = acc_pk(s.u_pk[0], x, 0, n_a);
                    if (ib == n_a) { close(s.u_pk[0]); s.u_pk[0] = splat(0.0f); }
                } else {
                    close(acc_pk(s.u_pk[0], x, 0, ib));
                    s.u_pk[0] = acc_pk(splat(0.0f), x, ib, n_a);
                }
                put_words(x, a0, n_a);
            }
            // (2) the launch's head: frames < dly come from the line (what the previous launch's last frames left there)
            v2f *pkp = lds_pk + (2 + o) * HALF + lane;
            if (head) {
                const int n_h = (size_t)dly - frame0 < (size_t)n ? (int)((size_t)dly - frame0) : n;
                v2f pk = (cq == 0) ? splat(0.0f) : *pkp;
                pk = acc_pk(pk, dl, 0, n_h);
                *pkp = pk;
                put_words(dl, frame0, n_h);
            }
            if (cq == g.cpb - 1 && (size_t)kq * g.B < (size_t)dly) {      // a packet with frames from the line ends
                const v2f pk = head ? *pkp : ((cq == 0) ? splat(0.0f) : *pkp);
                if ((size_t)(kq + 1u) * g.B <= (size_t)dly) finish_packet(kq, pk);
                else {
                    v2f m = pk;
#pragma unroll
                    for (int c = 0; c < 2; ++c) m[c] = fmaxf(pk[c], s.u_pk[1][c]);      // (meters are never NaN: peak_acc)
                    finish_packet(kq, m);
                }
            }
            // (3) the line keeps the launch's last max_delay frames
            // (non-temporal: nothing in this launch reads these rows again, nor the tiled words below — whole 512-byte rows per instruction, so
            //  nothing has to meet in L2 either; tiled words: 9.28 -> 8.96 ms on one box, a third of it from these rows)
            if (keep) rows_store<TAIL, true>(x, n, line, lane * 2, wb, dmask);
        } else if (dl_early) {
#ifdef DSPI_WAVE_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // timing build only: isolate the wait for the delayed rows
#endif
            WT_PHASE(3 + o, 1, WT_NOW() - wt1);
            [[maybe_unused]] const unsigned long long wt2 = WT_NOW();
            emit(dl);
            WT_PHASE(3 + o, 2, WT_NOW() - wt2);       // peaks + words + word stores
            [[maybe_unused]] const unsigned long long wt3 = WT_NOW();
            rows_store<TAIL>(x, n, line, lane * 2, wb, dmask);
            WT_PHASE(3 + o, 3, WT_NOW() - wt3);       // delay-line stores
        } else {
            emit(x);
        }
    }
    }      // work
    else if (sm_pair) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the launch's last steps: the last chunks' rows, as above)
    // ---- (stream-major pairs) this wave's half of the chunk to emit: meters, words, half a line per stream and pair buffer ----
    [[maybe_unused]] const unsigned long long wt4 = WT_NOW();
    if (emit_prev) {
        const int en = (TAIL ? (int)min((uint32_t)T, g.B - e_cq * T) : T) - eh * H;      // live frames of this half (<= 0: none)
        uint32_t stream_ = stream, lane_ = lane;
        asm volatile("" : "+v"(stream_), "+v"(lane_));      // (addresses formed per chunk, see the tiled layout's words)
        if (e_cq == 0) { s.u_pk[0] = splat(0.0f); s.u_pk[1] = splat(0.0f); }
#pragma unroll
        for (int side = 0; side < 2; ++side)
#pragma unroll
            for (int i = 0; i < H; i += 2) {      // usb_audio.c:915-923 (ragged chunk: frames past its end count as 0)
                const v2f y0 = (!TAIL || i < en) ? dl[side * H + i] : splat(0.0f), y1 = (!TAIL || i + 1 < en) ? dl[side * H + i + 1] : splat(0.0f);
                s.u_pk[side].x = peak_acc2(s.u_pk[side].x, y0.x, y1.x);
                s.u_pk[side].y = peak_acc2(s.u_pk[side].y, y0.y, y1.y);
            }
        if (e_cq == g.cpb - 1) {      // the packet ends: the partner's output's half goes to the mailbox, this wave's own is held for a step
            // (selected, not indexed: a run-time index would put the whole wave state into scratch memory)
            mail[((e_kq & 1u) * 8u + (uint32_t)(o ^ 1)) * 64u + lane_] = meter_word(eh ? s.u_pk[0] : s.u_pk[1]);
            s.u_w = meter_word(eh ? s.u_pk[1] : s.u_pk[0]);
        }
        if (a.pairs && !(DSPI_EXP_EMIT & 1)) {
            // a pair whose two outputs are both disabled is zero-filled whatever its lines still hold (usb_audio.c:930-933)
            const float scale = (((img->out_enabled >> o) | (img->out_enabled >> (o ^ 1))) & 1u) ? 8388607.0f : 0.0f;
            const bool shift = a.i2s_slots && ((img->i2s_pairs >> (o >> 1)) & 1u);      // an I2S slot's words leave left-justified (audio_i2s_multi.c:217-226)
            v2u w[T];
#pragma unroll
            for (int i = 0; i < T; ++i) {
                v2f d = v2f{clamp_pm1(dl[i].x), clamp_pm1(dl[i].y)} * scale;
                w[i] = v2u{(uint32_t)(int32_t)d.x, (uint32_t)(int32_t)d.y};
            }
            if (shift) {
#pragma unroll
                for (int i = 0; i < T; ++i) w[i] = w[i] << 8u;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                int32_t *dst = a.pairs + (((size_t)(stream_ + c - a.pairs_stream0) * P + (o >> 1)) * F + (size_t)e_kq * g.B + (size_t)e_cq * T + (size_t)eh * H) * 2;
#pragma unroll
                for (int j = 0; j < H / 2; ++j) {      // {L, R} of frames 2j, 2j + 1: w[i] = left side, w[H + i] = right side
                    // (non-temporal stores here: 34.7 ms instead of 10.4 — the line's eight 16-byte pieces, four from each wave of the pair, must meet in L2)
                    if (!TAIL || 2 * j + 1 < en) st4(dst + j * 4, u32x4{w[2 * j][c], w[H + 2 * j][c], w[2 * j + 1][c], w[H + 2 * j + 1][c]});
                    else if (2 * j < en) *reinterpret_cast<v2u *>(dst + j * 4) = v2u{w[2 * j][c], w[H + 2 * j][c]};
                }
            }
        }
    }
    if (emit_prev) WT_PHASE(3 + o, 3, WT_NOW() - wt4);       // emission: meters, words, line stores
    if ((DSPI_EXP_EMIT & 16) && sm_pair) {      // experiment: the previous step's rows drained at the END of this step, behind this step's own stores
        if (!TAIL && work && emit_prev && a.pairs) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");      // (16 row stores + 8 line stores of this step stay in flight)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (work && cq == g.cpb - 1 && (flags & IF_ANY_DELAY)) s.widx = (s.widx + g.B) & dmask;
}

// Stream-major words, the emission of whole pairs on a wave of its own (the master SIMD's third wave, otherwise idle).
// The per-wave timers of round 4 (profiles/r04_wave_timers_stream_split.log) show the two master waves busy for half of a step and the
// three-output SIMDs busy for all of it, a fifth to a third of that in the emission (row loads, conversions, line stores) and in the waits
// around it.  So the emission of the pairs in DSPI_EMIT_PAIRS — both halves of the frames, both sides — moves here: the rows of chunk q - 2
// of outputs 2p and 2p + 1 are read where output_item_pk's emit side finds them (delay line at frame - dly, or the mini line), metered
// (usb_audio.c:915-923), converted (:926-941) and written as whole [stream][pair][frame][2] lines (eight 16-byte stores per stream, all
// from this wave); a packet's peaks, clip bits and status slot are finished here too (no mailbox: this wave sees all sixteen frames of both
// outputs).  The pairs' own waves keep storing their rows and emit nothing.  `widx_e`: the lines' write index at the start of packet e_kq.
// pair_emit_load requests the rows of one pair (every pair's are requested before the first is used), pair_emit_finish does the rest.
template <bool TAIL>
__device__ __forceinline__ void pair_emit_load(const KArgs &a, ImgPtr img, const StateMap &sm, v2u widx_e, v2f (&dl)[2][T],
                                               uint32_t wg, uint32_t lane, int p, uint32_t e_cq, uint32_t e_q) {
    constexpr int N = make_state_map(1).n_out;
    const uint32_t flags = img->flags;
    const uint32_t dmask = (uint32_t)sm.max_delay - 1u;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int oo = 2 * p + side;
        const int32_t dly_ = img->delay_samples[oo];
        const bool dl_on_ = (flags & IF_ANY_DELAY) && dly_ > 0;
        const bool direct_ = dl_on_ && (dly_ >= sm.max_delay || dly_ <= sm.max_delay - 3 * T);      // (output_item_pk: e_direct)
        const uint32_t *src = direct_ ? a.dlines + ((size_t)wg * N + oo) * (size_t)sm.max_delay * ROWP
                                      : a.xwords + (((size_t)wg * 3 + (e_q % 3u)) * kMaxOut + oo) * (T * ROWP);
        const v2u pos = direct_ ? ((widx_e + e_cq * T - (uint32_t)dly_) & dmask) : v2u{0u, 0u};
        rows_load<TAIL, true>(dl[side], T, src, lane * 2, pos, direct_ ? dmask : (uint32_t)T - 1u);
    }
}
template <bool TAIL>
__device__ __forceinline__ void pair_emit_finish(const KArgs &a, ImgPtr img, const StateMap &sm, const Geo &g, const v2f (&dl)[2][T], v2f (&pk)[2], v2u &clip,
                                                 uint32_t wg, uint32_t lane, uint32_t stream, int p, uint32_t e_kq, uint32_t e_cq) {
    constexpr int P = make_state_map(1).n_pairs;
    const size_t F = (size_t)g.n_blocks * g.B;
    const int en = TAIL ? (int)min((uint32_t)T, g.B - e_cq * T) : T;      // live frames of the chunk
    uint32_t stream_ = stream, lane_ = lane;
    asm volatile("" : "+v"(stream_), "+v"(lane_));      // (addresses formed per chunk, see output_item_pk)
    if (e_cq == 0) { pk[0] = splat(0.0f); pk[1] = splat(0.0f); }
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int i = 0; i < T; i += 2) {      // usb_audio.c:915-923 (ragged chunk: frames past its end count as 0)
            const v2f y0 = live(dl[side][i], TAIL, i, en), y1 = live(dl[side][i + 1], TAIL, i + 1, en);
            pk[side].x = peak_acc2(pk[side].x, y0.x, y1.x);
            pk[side].y = peak_acc2(pk[side].y, y0.y, y1.y);
        }
    if (e_cq == g.cpb - 1) {      // the packet ends: peaks, sticky bits, status slot of the launch's last packet (usb_audio.c:915-923, :945-951)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int oo = 2 * p + side;
            v2u p16;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                p16[c] = (uint32_t)(fminf(1.0f, pk[side][c]) * 32767.0f);
                if (pk[side][c] > 1.001f) clip[c] |= 1u << (2 + oo);
                if (a.peaks) a.peaks[((size_t)(stream_ + c) * g.n_blocks + e_kq) * sm.n_ch + 2 + oo] = (uint16_t)p16[c];
            }
            if (e_kq == g.n_blocks - 1) *reinterpret_cast<v2u *>(a.state + ((size_t)wg * sm.n_slots + sm.peaks + 2 + oo) * ROWP + lane_ * 2) = p16;
        }
    }
    if (a.pairs) {
        // a pair whose two outputs are both disabled is zero-filled whatever its lines still hold (usb_audio.c:930-933)
        const float scale = ((img->out_enabled >> (2 * p)) & 3u) ? 8388607.0f : 0.0f;
        const bool shift = a.i2s_slots && ((img->i2s_pairs >> p) & 1u);      // an I2S slot's words leave left-justified (audio_i2s_multi.c:217-226)
        // frame pair by frame pair: four rows are converted and leave as one 16-byte store per stream — no array of words next to the rows
        // (two pairs' rows are in flight in this wave: 128 registers)
        int32_t *dst0 = a.pairs + (((size_t)(stream_ - a.pairs_stream0) * P + p) * F + (size_t)e_kq * g.B + (size_t)e_cq * T) * 2;
        int32_t *dst1 = dst0 + (size_t)P * F * 2;      // the lane's second stream
        auto word = [&](v2f y) {
            const v2f d = v2f{clamp_pm1(y.x), clamp_pm1(y.y)} * scale;
            v2u w = v2u{(uint32_t)(int32_t)d.x, (uint32_t)(int32_t)d.y};
            if (shift) w = w << 8u;
            return w;
        };
#pragma unroll
        for (int j = 0; j < T / 2; ++j) {      // {L, R} of frames 2j, 2j + 1
            const v2u l0 = word(dl[0][2 * j]), r0 = word(dl[1][2 * j]);
            if (!TAIL || 2 * j + 1 < en) {
                const v2u l1 = word(dl[0][2 * j + 1]), r1 = word(dl[1][2 * j + 1]);
                // (non-temporal stores here: 24.4 ms instead of 10.6 — 16-byte pieces do not combine on that path even when one wave writes
                //  all eight pieces of a line back to back; profiles/r05_headline_experiments.md)
                st4(dst0 + j * 4, u32x4{l0.x, r0.x, l1.x, r1.x});
                st4(dst1 + j * 4, u32x4{l0.y, r0.y, l1.y, r1.y});
            } else if (2 * j < en) {
                *reinterpret_cast<v2u *>(dst0 + j * 4) = v2u{l0.x, r0.x};
                *reinterpret_cast<v2u *>(dst1 + j * 4) = v2u{l0.y, r0.y};
            }
        }
    }
}
// ---- the emitter wave, whole pair-buffer lines: pair_lines_load / pair_lines_finish / pair_lines_packet_end ----
// A line of the stream-major pair buffer is sixteen frames of ONE stream ({L, R} x 16 = 128 bytes).  In the row mapping above a lane holds two
// streams and all sixteen frames, so each of its 16-byte stores lands in 64 different lines and the pieces have to meet in L2.  The emitter
// wave owns no output, it only READS rows, so it may read them in the mapping the STORES want: lane = (g = lane >> 3, j = lane & 7), j the
// frame pair of the chunk; for u = 0..3 the lane serves the stream quad 8u + g of the row (streams 4(8u + g) .. + 3).  One 16-byte load at
// row 2j + e, words 4(8u + g) .. + 3, gives the lane four adjacent streams of one frame; the 4 x 4 transposition to "four words of one
// stream" is register naming.  Per instruction: eight rows x one full 128-byte line (eight g), 16 instructions per pair — 128 line requests,
// the figure of the 32 row loads of pair_emit_load.  A stream's piece {L 2j, R 2j, L 2j+1, R 2j+1} then leaves as one 16-byte store; eight
// adjacent lanes (j) write one whole line and an instruction writes eight whole lines, so the stores can be non-temporal (a PARTIAL line
// stored non-temporally is the 24 ms case noted in pair_emit_finish: the path is taken only where every line is whole and aligned).
// The rows were written by other waves of the workgroup: every load bypasses the CU's L1 (aux 16 = sc1, what ld_agent2 does), as a raw
// buffer load whose descriptor is wave-uniform (one per (row, output) line or mini line; offsets past the line read as zero, never fault).
// Running packet peaks would need a register per (stream, side) here; they live in LDS instead (ds_max_u32 on the non-negative float's bit
// pattern, which orders like an integer): `acc` [pair][side][128], the area of the posted envelopes, which only the split master of the
// per-lane-filter kernels uses — and that instantiation has no emitter wave.
// Needs: all 128 streams of the row in the launch, at ONE line write position w0, whole 16-frame chunks (not TAIL), 128-byte aligned lines.
__device__ __forceinline__ void pair_lines_load(const KArgs &a, ImgPtr img, const StateMap &sm, uint32_t w0, u32x4 (&v)[2][2][4],
                                                uint32_t wg, uint32_t lane, int p, uint32_t e_cq, uint32_t e_q) {
    constexpr int N = make_state_map(1).n_out;
    const uint32_t flags = img->flags;
    const uint32_t dmask = (uint32_t)sm.max_delay - 1u;
    uint32_t g8 = lane >> 3, j8 = lane & 7u;
    asm volatile("" : "+v"(g8), "+v"(j8));      // (addresses formed per chunk, see output_item_pk)
    __amdgpu_buffer_rsrc_t rs[2];
    uint32_t off[2][2];      // byte offset of the lane's first quad in row 2j + e of each side
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int oo = 2 * p + side;
        const int32_t dly_ = img->delay_samples[oo];
        const bool dl_on_ = (flags & IF_ANY_DELAY) && dly_ > 0;
        const bool direct_ = dl_on_ && (dly_ >= sm.max_delay || dly_ <= sm.max_delay - 3 * T);      // (output_item_pk: e_direct)
        uint32_t *src = direct_ ? a.dlines + ((size_t)wg * N + oo) * (size_t)sm.max_delay * ROWP
                                : a.xwords + (((size_t)wg * 3 + (e_q % 3u)) * kMaxOut + oo) * (T * ROWP);
        rs[side] = __builtin_amdgcn_make_buffer_rsrc(src, 0, (int)((direct_ ? (uint32_t)sm.max_delay : (uint32_t)T) * ROWP * 4u), 0x00020000);
        const uint32_t pos0 = direct_ ? w0 + e_cq * T - (uint32_t)dly_ : 0u, pm = direct_ ? dmask : (uint32_t)T - 1u;
#pragma unroll
        for (int e = 0; e < 2; ++e) off[side][e] = (((pos0 + 2u * j8 + (uint32_t)e) & pm) * ROWP + 4u * g8) * 4u;      // (the mask per row: a chunk may wrap inside the line)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)      // quad by quad, the order pair_lines_finish uses them in
#pragma unroll
        for (int side = 0; side < 2; ++side)
#pragma unroll
            for (int e = 0; e < 2; ++e) v[side][e][u] = __builtin_amdgcn_raw_buffer_load_b128(rs[side], (int)(off[side][e] + (uint32_t)u * 128u), 0, 16);
}
__device__ __forceinline__ void pair_lines_finish(const KArgs &a, ImgPtr img, const Geo &g, const u32x4 (&v)[2][2][4], uint32_t *__restrict__ acc,
                                                  uint32_t wg, uint32_t lane, int p, uint32_t e_kq, uint32_t e_cq) {
    constexpr int P = make_state_map(1).n_pairs;
    const size_t F = (size_t)g.n_blocks * g.B;
    uint32_t g8 = lane >> 3, j8 = lane & 7u;
    asm volatile("" : "+v"(g8), "+v"(j8));      // (addresses formed per chunk, see output_item_pk)
    // a pair whose two outputs are both disabled is zero-filled whatever its lines still hold (usb_audio.c:930-933)
    const float scale = ((img->out_enabled >> (2 * p)) & 3u) ? 8388607.0f : 0.0f;
    const bool shift = a.i2s_slots && ((img->i2s_pairs >> p) & 1u);      // an I2S slot's words leave left-justified (audio_i2s_multi.c:217-226)
    auto word = [&](uint32_t l, uint32_t r) {      // {L, R} of one frame, exactly pair_emit_finish's word
        const v2f d = v2f{clamp_pm1(as_f(l)), clamp_pm1(as_f(r))} * scale;
        v2u w = v2u{(uint32_t)(int32_t)d.x, (uint32_t)(int32_t)d.y};
        if (shift) w = w << 8u;
        return w;
    };
    int32_t *dst = a.pairs ? a.pairs + (((size_t)(wg * ROWP + 4u * g8 - a.pairs_stream0) * P + p) * F + (size_t)e_kq * g.B + (size_t)e_cq * T + 2u * j8) * 2 : nullptr;
    const size_t sstride = (size_t)P * F * 2;      // words from a stream to the next
    uint32_t *m = acc + 4u * g8;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // meters (usb_audio.c:915-923): max(|y 2j|, |y 2j+1|) into the stream's packet peak; a NaN leaves a meter alone, as peak_acc does
            float ml, mr;
            asm("v_max3_f32 %0, |%1|, |%2|, 0" : "=v"(ml) : "v"(as_f(v[0][0][u][k])), "v"(as_f(v[0][1][u][k])));
            asm("v_max3_f32 %0, |%1|, |%2|, 0" : "=v"(mr) : "v"(as_f(v[1][0][u][k])), "v"(as_f(v[1][1][u][k])));
            atomicMax(m + (32 * u + k), as_u(ml));
            atomicMax(m + (ROWP + 32 * u + k), as_u(mr));
            if (dst) {
                const v2u f0 = word(v[0][0][u][k], v[1][0][u][k]), f1 = word(v[0][1][u][k], v[1][1][u][k]);
                // eight adjacent lanes: one whole line that nobody here reads again
                __builtin_nontemporal_store(u32x4{f0.x, f0.y, f1.x, f1.y}, reinterpret_cast<u32x4 *>(dst + (size_t)(32 * u + k) * sstride));
            }
        }
}
// a packet ends: the LDS meters of pair p become peaks, sticky bits and the status slot of the launch's last packet (usb_audio.c:915-923,
// :945-951), and are cleared for the next packet.  Lane l finishes streams l and l + 64 of the row.
__device__ __forceinline__ void pair_lines_packet_end(const KArgs &a, const StateMap &sm, const Geo &g, uint32_t *__restrict__ acc, v2u &clip,
                                                      uint32_t wg, uint32_t lane, int p, uint32_t e_kq) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int oo = 2 * p + side;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t col = lane + 64u * (uint32_t)h;
            asm volatile("" : "+v"(col));      // (addresses formed per packet)
            const float pk = as_f(acc[side * ROWP + col]);
            acc[side * ROWP + col] = 0u;
            const uint32_t p16 = (uint32_t)(fminf(1.0f, pk) * 32767.0f);
            if (pk > 1.001f) clip[h] |= 1u << (2 + oo);
            if (a.peaks) a.peaks[((size_t)(wg * ROWP + col) * g.n_blocks + e_kq) * sm.n_ch + 2 + oo] = (uint16_t)p16;
            if (e_kq == g.n_blocks - 1) a.state[((size_t)wg * sm.n_slots + sm.peaks + 2 + oo) * ROWP + col] = p16;
        }
    }
}
// the pairs of a mask, lowest first (compile-time)
constexpr int emit_pair_count(unsigned m) { return m ? 1 + emit_pair_count(m & (m - 1)) : 0; }
constexpr int emit_pair_nth(unsigned m, int n) { return n == 0 ? __builtin_ctz(m | 0x100u) : emit_pair_nth(m & (m - 1), n - 1); }

// ==========================================================================================
// the packed kernel: 12 waves = 768 threads, 128 streams per workgroup, one workgroup per CU (LDS)
// ==========================================================================================
// Role table, wave -> work.  Twelve waves; waves w, w+4, w+8 share a SIMD (measured: HW_ID.SIMD_ID), and a dependent
// v_pk op issues ~16 cycles after its producer (tools/probe/probe5), so a wave alone on a SIMD runs the band
// recurrences chain-bound while three waves keep the SIMD issuing and cover each other's memory stalls.
//   SIMD a: wave 0 = master intake (input, loudness, master EQ, leveller pass 1 -> ring), wave 4 = master hand-off
//           (ring -> leveller pass 2, peaks, crossfeed -> LDS), wave 8 idle.  With the leveller off wave 0 does both.
//   SIMD b/c/d: one output per wave, outputs o, o+3, o+6 together (the three heaviest EQ sets on different SIMDs).
struct PkRole { int kind, o; };     // kind 0 intake(+hand-off), 1 hand-off, 2 idle, 3 output
// r = position of the wave in (SIMD, arrival) order: waves that share a SIMD get consecutive r (see the kernel prologue)
__device__ __forceinline__ PkRole pk_role(int r) {
    const int grp = r / 3, k = r % 3;
    if (grp == 0) return {k, 0};
    return {3, (grp - 1) + 3 * k};
}
constexpr int kPkWaves = 12;

// Specialised on what the host knows per launch (tail packets, leveller on/off for this image, input word size, output
// layout): fewer live alternatives for the register allocator, which is at the 168-VGPR limit of 3 waves per SIMD.
// PV: per-lane values (numbers from the row's value tile); PVB: the band coefficients too (PV alone: the row's presets differ only in
// gains, volumes, leveller / crossfeed numbers — their filters are identical, the shared-coefficient band loops serve them)
template <bool TAIL, bool LEV, bool PCM24, bool TILED, bool FMA, bool PV = false, bool PVB = false>
__global__ __launch_bounds__(64 * kPkWaves, 1) void chain_kernel_pk(KArgs a) {
    constexpr StateMap sm = make_state_map(1);
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    v2f *lds_state = reinterpret_cast<v2f *>(lds);                          // [lds_slots][64] v2f
    v2f *lds_pk = lds_state + sm.lds_slots * HALF;                          // [n_ch][64]
    v2f *xch = lds_pk + sm.n_ch * HALF;                                     // [2][2][T][64]
    v2f *mailbox = xch + 2 * 2 * T * HALF;                                  // [kMailbox][64]

    const WgItem item = a.items[blockIdx.x];
    const uint32_t wg = item.wg;
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t stream = wg * ROWP + lane * 2;       // first of the lane's two streams
    asm volatile("s_mov_b64 exec, %0" ::"s"(item.mask) : "memory");   // see chain_kernel
    ImgPtr img = to_const(a.img + item.image);
    const float *tile = PV ? a.vals + (size_t)wg * kPvTileFloats : nullptr;      // wave-uniform

    uint32_t *gs = a.state + (size_t)wg * sm.n_slots * ROWP + lane * 2;
    v2u *lds2 = reinterpret_cast<v2u *>(lds);
    for (int s = wave; s < sm.lds_slots; s += kPkWaves) lds2[s * HALF + lane] = *reinterpret_cast<const v2u *>(gs + (size_t)s * ROWP);
    // Roles by SIMD.  Where the CU puts the twelve waves is not a function of the wave index (it depends on what is still
    // draining from the previous workgroup), so each wave looks up its SIMD (HW_ID[5:4]) and takes the next role of that
    // SIMD's group: {intake, hand-off, idle} on one SIMD, three outputs on each of the others.  Uneven placements
    // (4/2/3/3 ...) still get every role exactly once, just with a group spilling over to a neighbour.
    uint32_t *role_cnt = reinterpret_cast<uint32_t *>(mailbox + kMailbox * HALF);      // [4]
    v2f *envpost = mailbox + kMailbox * HALF + 2;                                      // [2][2][64] left / right envelope at packet end (per-lane filters: intake and third wave -> hand-off wave)
    const uint32_t first_lane = (uint32_t)__builtin_ctzll(item.mask);        // EXEC is narrowed: only lanes of the mask run
    if (wave == 0 && lane == first_lane) { role_cnt[0] = 0; role_cnt[1] = 0; role_cnt[2] = 0; role_cnt[3] = 0; }
    __syncthreads();
    const uint32_t simd = (__builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11))) & 3u;   // hwreg(HW_REG_HW_ID, 4, 2)
    uint32_t slot = 0;
    if (lane == first_lane) slot = atomicAdd(&role_cnt[simd], 1u);
    slot = __builtin_amdgcn_readlane(slot, first_lane);
    __syncthreads();
    uint32_t rank = slot;
    for (uint32_t q = 0; q < simd; ++q) rank += role_cnt[q];
    rank = __builtin_amdgcn_readfirstlane(rank);
    auto ld2 = [&](int slot) { return *reinterpret_cast<const v2u *>(gs + (size_t)slot * ROWP); };
    auto st2 = [&](int slot, v2u v) { *reinterpret_cast<v2u *>(gs + (size_t)slot * ROWP) = v; };

    Geo g;
    g.n_blocks = a.n_blocks; g.B = a.block_len;
    g.cpb = (g.B + T - 1) / T;
    g.items = g.n_blocks * g.cpb;
    // hand-off of chunk q happens at step q + lag: a packet later for the leveller (its ramp is known when pass 1 of the
    // packet has ended), and never sooner than 3 steps, which is what makes the intake wave's ring rows visible to the
    // hand-off wave's prefetch one step before use (see master_intake_pk)
    g.lag = LEV ? (g.cpb > 3u ? g.cpb : 3u) : 0u;
    // stream-major words: one pair's emission runs on the master SIMD's third wave (pair_emit_step) unless that wave carries the right master
    // channel (per-lane master filters with the leveller on)
    constexpr bool ext_emit = !TILED && !(PVB && LEV) && (DSPI_EMIT_PAIRS) != 0;
    constexpr unsigned ext_mask = ext_emit ? (unsigned)(DSPI_EMIT_PAIRS) & 0xfu : 0u;
    constexpr bool xcopy = !TILED;      // stream-major words: a pair's two waves emit a chunk two steps after they stored its rows (output_item_pk), so the launch is two steps longer; the last packet's meters are finished behind the loop's last barrier
    g.steps = g.items + g.lag + 1 + (xcopy ? 2u : 0u);
    const PkRole role = pk_role((int)rank);
    uint32_t *ring = a.ring + (size_t)wg * kRingLen * 2 * ROWP;      // wave-uniform; the lane offset goes into the accesses
    uint32_t *ring_r = ring + (size_t)kRingLen * ROWP;

    if (role.kind == 0) {
        // ---- master intake (and, leveller off, the hand-off too) ----
        MasterPk m;
        m.lpL = as_v2f(ld2(sm.xfeed + 0)); m.lpR = as_v2f(ld2(sm.xfeed + 1));
        m.apL = as_v2f(ld2(sm.xfeed + 2)); m.apR = as_v2f(ld2(sm.xfeed + 3));
        m.env_l = as_v2f(ld2(sm.lev + 0)); m.env_r = as_v2f(ld2(sm.lev + 1));
        m.gsm_db = as_v2f(ld2(sm.lev + 2)); m.g_cur = as_v2f(ld2(sm.lev + 3)); m.g_prev = as_v2f(ld2(sm.lev + 4));
        m.rp1 = m.rp2 = ld2(sm.ring_pos) & (uint32_t)(kRingLen - 1);
        m.p2_gain = splat(1.0f); m.p2_step = splat(0.0f); m.g_last = m.g_cur; m.pk_l = m.pk_r = splat(0.0f);
        m.pre_valid = 0;
#pragma unroll
        for (int v = 0; v < T / 4; ++v) { m.pre[0][v] = u32x4{0, 0, 0, 0}; m.pre[1][v] = u32x4{0, 0, 0, 0}; }
        m.clip = LEV ? v2u{0u, 0u} : ld2(sm.clip + 0);
        uint32_t k1 = 0, c1 = 0;
        v2f xl[T], xr[T];
#pragma unroll
        for (int i = 0; i < T; ++i) { xl[i] = splat(0.0f); xr[i] = splat(0.0f); }
        bool master_differ = false;
        if constexpr (PVB) master_differ = (pv_differ(tile, 0, 2 * kBands) | pv_differ(tile, kMaxCh * kBands, 2)) != 0u;
        // per-lane master filters, leveller on: this wave runs the LEFT channel, the hand-off wave the right one and the gain decision
        const bool split = PVB && LEV && master_differ;
        WT_DECL;
        for (uint32_t st = 0; st < g.steps; ++st) {
            if (st < g.items) {
                if (split) {
                    if constexpr (PVB && LEV) master_intake_pv<TAIL, PCM24, FMA>(a, img, tile, sm, g, m, xl, lds_state, mailbox, envpost, ring, ring_r, lane, stream, k1, c1, 1);
                } else if (PVB && !LEV && master_differ) {
                    if constexpr (PVB && !LEV) {      // per-lane master filters, leveller off: the channels one after the other, parked in LDS
                        v2f *park = xch + (size_t)(st & 1u) * (2 * T * HALF) + lane;
                        master_intake_pv<TAIL, PCM24, FMA>(a, img, tile, sm, g, m, xl, lds_state, mailbox, envpost, ring, ring_r, lane, stream, k1, c1, 0, park);
#pragma unroll
                        for (int i = 0; i < T; ++i) { xl[i] = park[i * HALF]; xr[i] = park[(T + i) * HALF]; }
                    }
                } else master_intake_pk<TAIL, PCM24, FMA, PV, PVB>(a, img, tile, sm, g, m, xl, xr, lds_state, mailbox, ring, ring_r, lane, stream, LEV, k1, c1);
                if (!LEV) master_handoff_pk<TAIL, FMA, PV>(a, img, tile, sm, g, m, xl, xr, xch, mailbox, wg, lane, stream, false, k1, c1, st);
                if (!PV) master_prefetch_pk<TAIL, PCM24>(a, g, m, stream, k1, c1);      // (per-lane values: the registers go to the value pairs; a spilled dword costs a 256-byte row of traffic per access)
                if (++c1 == g.cpb) { c1 = 0; ++k1; }
            } else if (LEV) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the last chunks' ring rows, see master_intake_pk
            }
            WT_BEFORE_BARRIER;
            lds_barrier();
            WT_AFTER_BARRIER;
        }
        WT_FINISH(rank);
        if (!LEV) {
            st2(sm.xfeed + 0, as_v2u(m.lpL)); st2(sm.xfeed + 1, as_v2u(m.lpR));
            st2(sm.xfeed + 2, as_v2u(m.apL)); st2(sm.xfeed + 3, as_v2u(m.apR));
            st2(sm.clip + 0, m.clip);
        }
        st2(sm.lev + 0, as_v2u(m.env_l));
        if (!split) {      // (split: the hand-off wave carries these)
            st2(sm.lev + 1, as_v2u(m.env_r));
            st2(sm.lev + 2, as_v2u(m.gsm_db)); st2(sm.lev + 3, as_v2u(m.g_cur)); st2(sm.lev + 4, as_v2u(m.g_prev));
        }
        st2(sm.ring_pos, m.rp1);
    } else if (role.kind == 1 && LEV) {
        // ---- master hand-off (leveller on): ring -> pass 2 -> peaks -> crossfeed -> LDS, one packet (>= 3 steps) late ----
        MasterPk m;
        m.lpL = as_v2f(ld2(sm.xfeed + 0)); m.lpR = as_v2f(ld2(sm.xfeed + 1));
        m.apL = as_v2f(ld2(sm.xfeed + 2)); m.apR = as_v2f(ld2(sm.xfeed + 3));
        m.g_last = as_v2f(ld2(sm.lev + 3));
        m.rp2 = ld2(sm.ring_pos) & (uint32_t)(kRingLen - 1);
        m.p2_gain = splat(1.0f); m.p2_step = splat(0.0f); m.pk_l = m.pk_r = splat(0.0f);
        m.clip = ld2(sm.clip + 0);
        uint32_t kq = 0, cq = 0;
        v2f xl[T], xr[T];
#pragma unroll
        for (int i = 0; i < T; ++i) { xl[i] = splat(0.0f); xr[i] = splat(0.0f); }
        // per-lane master filters: pass 1 of the two channels runs on the other two waves of this SIMD (left: intake wave, right: the
        // third wave); each posts its flushed end-of-packet envelope before the barrier of the step that ended the packet, and this wave
        // takes the packet's gain decision at the start of the next step.  The decision precedes, in program order, the hand-off that
        // uses it (lag >= a packet).
        bool split = false;
        if constexpr (PVB) split = (pv_differ(tile, 0, 2 * kBands) | pv_differ(tile, kMaxCh * kBands, 2)) != 0u;
        uint32_t k1 = 0, c1 = 0, kd = 0;
        bool decide = false;
        m.env_l = splat(0.0f); m.env_r = splat(0.0f); m.gsm_db = splat(0.0f); m.g_cur = splat(1.0f); m.g_prev = splat(1.0f); m.rp1 = m.rp2;
        if (split) { m.gsm_db = as_v2f(ld2(sm.lev + 2)); m.g_cur = as_v2f(ld2(sm.lev + 3)); m.g_prev = as_v2f(ld2(sm.lev + 4)); }
        WT_DECL;
        for (uint32_t st = 0; st < g.steps; ++st) {
            if constexpr (PVB) {
                if (split && decide) {
                    m.env_r = envpost[(2 + (kd & 1u)) * HALF + lane];
                    pv_gain_decision<FMA>(tile, lane, m, envpost[(kd & 1u) * HALF + lane], g.B, mailbox, kd);
                    decide = false;
                }
            }
            if (st >= g.lag && st < g.items + g.lag) {
                master_handoff_pk<TAIL, FMA, PV>(a, img, tile, sm, g, m, xl, xr, xch, mailbox, wg, lane, stream, true, kq, cq, st - g.lag);
                if (++cq == g.cpb) { cq = 0; ++kq; }
            }
            if (PVB && split && st < g.items) { if (++c1 == g.cpb) { decide = true; kd = k1; c1 = 0; ++k1; } }
            // rows for the next step's hand-off: stored by the intake wave >= 2 steps ago, requested a full step early
            if (st + 1 >= g.lag && st + 1 < g.items + g.lag) master_fetch_pk<TAIL>(img, g, m, xl, xr, ring, ring_r, lane, cq);
            WT_BEFORE_BARRIER;
            lds_barrier();
            WT_AFTER_BARRIER;
        }
        WT_FINISH(rank);
        st2(sm.xfeed + 0, as_v2u(m.lpL)); st2(sm.xfeed + 1, as_v2u(m.lpR));
        st2(sm.xfeed + 2, as_v2u(m.apL)); st2(sm.xfeed + 3, as_v2u(m.apR));
        st2(sm.clip + 0, m.clip);
        if (split) { st2(sm.lev + 2, as_v2u(m.gsm_db)); st2(sm.lev + 3, as_v2u(m.g_cur)); st2(sm.lev + 4, as_v2u(m.g_prev)); }
    } else if (role.kind == 2 && PVB && LEV) {
        // ---- third wave of the master SIMD: per-lane master filters with the leveller on — pass 1 of the RIGHT channel (the left one runs
        // on the intake wave) ----
        bool rsplit = false;
        if constexpr (PVB && LEV) rsplit = (pv_differ(tile, 0, 2 * kBands) | pv_differ(tile, kMaxCh * kBands, 2)) != 0u;
        MasterPk m;
        m.env_l = splat(0.0f); m.env_r = splat(0.0f);
        m.rp1 = v2u{0u, 0u};
        if (rsplit) { m.env_r = as_v2f(ld2(sm.lev + 1)); m.rp1 = ld2(sm.ring_pos) & (uint32_t)(kRingLen - 1); }
        v2f xr[T];
#pragma unroll
        for (int i = 0; i < T; ++i) xr[i] = splat(0.0f);
        uint32_t k1 = 0, c1 = 0;
        WT_DECL;
        for (uint32_t st = 0; st < g.steps; ++st) {
            if constexpr (PVB && LEV) {
                if (rsplit) {
                    if (st < g.items) {
                        master_intake_pv<TAIL, PCM24, FMA>(a, img, tile, sm, g, m, xr, lds_state, mailbox, envpost, ring, ring_r, lane, stream, k1, c1, 2);
                        if (++c1 == g.cpb) { c1 = 0; ++k1; }
                    } else {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the last chunks' right rows
                    }
                }
            }
            WT_BEFORE_BARRIER;
            lds_barrier();
            WT_AFTER_BARRIER;
        }
        WT_FINISH(rank);
        if (rsplit) st2(sm.lev + 1, as_v2u(m.env_r));
    } else if (role.kind == 2 && ext_emit) {
        // ---- third wave of the master SIMD, stream-major words: the emission of the pairs in DSPI_EMIT_PAIRS ----
        // whole lines (pair_lines_*) where the row allows it, else the row mapping (pair_emit_load / _finish)
        constexpr int NP = emit_pair_count(ext_mask);
        v2u widx_e = ld2(sm.widx);
        uint32_t e_kq = 0, e_cq = 0;
        asm volatile("" : "+v"(widx_e));      // (arrived before the time loop: see the output waves below)
        const uint32_t dmask = (uint32_t)sm.max_delay - 1u;
        // Whole lines: decided once, wave-uniform.  The whole row is in the launch, its 128 streams share one line write position, the chunks
        // are whole (not TAIL), and every line of the pair buffer is 128-byte aligned (or there is no pair buffer: meters only).
        static_assert(NP * 2 * ROWP * sizeof(uint32_t) <= 2 * 2 * HALF * sizeof(v2f), "the emitter wave's LDS meters: two pairs fit the posted envelopes' area");
        uint32_t *acc = reinterpret_cast<uint32_t *>(envpost);      // [NP][2 sides][128 streams] running packet peaks (float bits)
        uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)widx_e.x);
        const bool lines = !TAIL && !a.no_emit_lines && item.mask == ~0ull && __all(widx_e.x == widx_e.y && widx_e.x == w0) &&
                           (!a.pairs || ((reinterpret_cast<uintptr_t>(a.pairs) & 127u) == 0 && (g.n_blocks * g.B) % 16u == 0));
        // (a time loop each: one loop with both bodies hoists the addresses of both and spills them)
        if (lines) {
            if constexpr (!TAIL) {
#pragma unroll
                for (int i = 0; i < NP * 2 * 2; ++i) acc[i * 64 + lane] = 0u;
                v2u clip = v2u{0u, 0u};
                WT_DECL;
                for (uint32_t st = 0; st < g.steps; ++st) {
                    const uint32_t q = st - g.lag - 1;
                    if (st >= g.lag + 3 && q - 2u < g.items) {      // chunk q - 2: its rows are complete behind the barrier that ended step st - 1 (output_item_pk)
                        // two pairs' rows in flight at most (128 of the wave's registers): pair j + 1 is requested before pair j is converted and stored
                        u32x4 v[NP > 0 ? NP : 1][2][2][4];
                        if (NP > 0) pair_lines_load(a, img, sm, w0, v[0], wg, lane, emit_pair_nth(ext_mask, 0), e_cq, q - 2u);
#pragma unroll
                        for (int j = 0; j < NP; ++j) {
                            if (j + 1 < NP) pair_lines_load(a, img, sm, w0, v[j + 1], wg, lane, emit_pair_nth(ext_mask, j + 1), e_cq, q - 2u);
                            pair_lines_finish(a, img, g, v[j], acc + j * 2 * ROWP, wg, lane, emit_pair_nth(ext_mask, j), e_kq, e_cq);
                        }
                        if (++e_cq == g.cpb) {
#pragma unroll
                            for (int j = 0; j < NP; ++j) pair_lines_packet_end(a, sm, g, acc + j * 2 * ROWP, clip, wg, lane, emit_pair_nth(ext_mask, j), e_kq);
                            e_cq = 0; ++e_kq;
                            if (img->flags & IF_ANY_DELAY) w0 = (w0 + g.B) & dmask;      // (usb_audio.c:911)
                        }
                    }
                    WT_BEFORE_BARRIER;
                    lds_barrier();
                    WT_AFTER_BARRIER;
                }
                WT_FINISH(rank);
                uint32_t *cs = a.state + ((size_t)wg * sm.n_slots + sm.clip + 1) * ROWP + lane;      // (clip slots 1..3 are OR-ed by the reader; lane l: streams l and l + 64)
                atomicOr(cs, clip.x);
                atomicOr(cs + 64, clip.y);
            }
        } else {
            v2u clip = v2u{0u, 0u};
            v2f pk[NP > 0 ? NP : 1][2];
#pragma unroll
            for (int j = 0; j < NP; ++j) { pk[j][0] = splat(0.0f); pk[j][1] = splat(0.0f); }
            WT_DECL;
            for (uint32_t st = 0; st < g.steps; ++st) {
                const uint32_t q = st - g.lag - 1;
                if (st >= g.lag + 3 && q - 2u < g.items) {      // chunk q - 2, as above
                    // two pairs' rows in flight at most (128 of the wave's registers): pair j + 1 is requested before pair j is converted and stored
                    v2f dl[NP > 0 ? NP : 1][2][T];
                    if (NP > 0) pair_emit_load<TAIL>(a, img, sm, widx_e, dl[0], wg, lane, emit_pair_nth(ext_mask, 0), e_cq, q - 2u);
#pragma unroll
                    for (int j = 0; j < NP; ++j) {
                        if (j + 1 < NP) pair_emit_load<TAIL>(a, img, sm, widx_e, dl[j + 1], wg, lane, emit_pair_nth(ext_mask, j + 1), e_cq, q - 2u);
                        pair_emit_finish<TAIL>(a, img, sm, g, dl[j], pk[j], clip, wg, lane, stream, emit_pair_nth(ext_mask, j), e_kq, e_cq);
                    }
                    if (++e_cq == g.cpb) {
                        e_cq = 0; ++e_kq;
                        if (img->flags & IF_ANY_DELAY) widx_e = (widx_e + g.B) & dmask;      // (usb_audio.c:911)
                    }
                }
                WT_BEFORE_BARRIER;
                lds_barrier();
                WT_AFTER_BARRIER;
            }
            WT_FINISH(rank);
            atomicOr(gs + (size_t)(sm.clip + 1) * ROWP, clip.x);      // (clip slots 1..3 are OR-ed by the reader)
            atomicOr(gs + (size_t)(sm.clip + 1) * ROWP + 1, clip.y);
        }
    } else if (role.kind != 3) {
        for (uint32_t st = 0; st < g.steps; ++st) lds_barrier();      // idle partner: keeps the barrier count
    } else {
        OutPk s;
        s.widx = ld2(sm.widx);
        s.loading = ld2(sm.mute + 0); s.counter = ld2(sm.mute + 1); s.smooth = as_v2f(ld2(sm.mute + 2));
        s.vmm = splat(0.0f);
        s.clip = v2u{0u, 0u};          // OR-ed into the stream's sticky bits at the end (several waves share a clip slot)
        s.u_pk[0] = s.u_pk[1] = splat(0.0f); s.u_w = 0u;
        const OutConst<PV> oc = load_out_const<PV>(img, tile, lane, role.o, g.B);
        if (!(xcopy && role.o != sm.n_out - 1)) s.u_w = oc.dly_k;      // (words written ahead start in the delay's packet)
        uint32_t kq = 0, cq = 0, e_kq = 0, e_cq = 0, fin_k = 0;
        bool fin_prev = false;
        // The wave state loaded above must have ARRIVED before the time loop: otherwise the compiler's wait for it (vmcnt(3): "all but the three
        // loads issued after it") sits at its first use INSIDE the loop and runs every step — where it waits for the previous step's row and line
        // stores, the very wait the mid-step drain exists to avoid (found with a top-of-step timer: 2 000-3 300 cycles per step).
        // An empty asm that USES the loaded registers puts the compiler's wait here, in front of the loop.
#ifndef DSPI_NO_TOPUSE
        asm volatile("" : "+v"(s.widx), "+v"(s.loading), "+v"(s.counter), "+v"(s.smooth));
#endif
        // stream-major pairs: chunk q - 2 is emitted next to chunk q's EQ (output_item_pk) — but for the pair that the master SIMD's third wave emits
        const bool emits = xcopy && role.o != sm.n_out - 1 && !((ext_mask >> (role.o >> 1)) & 1u);
        WT_DECL;
        for (uint32_t st = 0; st < g.steps; ++st) {
            const uint32_t q = st - g.lag - 1;
            const bool work = st >= g.lag + 1 && q < g.items, emit_prev = emits && st >= g.lag + 3 && q - 2u < g.items;
            if (work || emit_prev || fin_prev) {
                output_item_pk<TAIL, TILED, FMA, PV, PVB>(a, img, tile, oc, sm, g, s, lds_state, lds_pk, xch, wg, lane, stream, role.o, kq, cq, q, work, emit_prev, e_kq, e_cq, fin_prev, fin_k);
                fin_prev = emit_prev && e_cq == g.cpb - 1; fin_k = e_kq;      // the packet that just ended is finished next step, when the partner's half has arrived
                if (work && ++cq == g.cpb) { cq = 0; ++kq; }
                if (emit_prev && ++e_cq == g.cpb) { e_cq = 0; ++e_kq; }
            } else if (xcopy && role.o != sm.n_out - 1 && !emits && st == g.lag + 1 + g.items) {
                // a pair the emitter wave serves: this wave never enters output_item_pk's tail (no emission of its own), so the rows of the
                // launch's LAST chunk are drained here, before the barrier that publishes them to the emitter wave (step items + lag + 2)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            WT_BEFORE_BARRIER;
            lds_barrier();
            WT_AFTER_BARRIER;
        }
        WT_FINISH(rank);
        // (stream-major pairs: the launch's last packet — its partner's half was posted before the loop's last barrier)
        if (fin_prev) output_item_pk<TAIL, TILED, FMA, PV, PVB>(a, img, tile, oc, sm, g, s, lds_state, lds_pk, xch, wg, lane, stream, role.o, kq, cq, g.items + 2u, false, false, e_kq, e_cq, true, fin_k);
        if (role.o == 0) {
            st2(sm.widx, s.widx);
            st2(sm.mute + 0, s.loading); st2(sm.mute + 1, s.counter); st2(sm.mute + 2, as_v2u(s.smooth));
        }
        // clip slots 1..3 are OR-ed by the reader (dspi_capi.cpp fetch_status); the nine output waves share them
        const int cslot = sm.clip + 1 + (role.o % 3);
        atomicOr(gs + (size_t)cslot * ROWP, s.clip.x);
        atomicOr(gs + (size_t)cslot * ROWP + 1, s.clip.y);
    }
    __syncthreads();
    for (int s = wave; s < sm.lds_slots; s += kPkWaves) *reinterpret_cast<v2u *>(gs + (size_t)s * ROWP) = lds2[s * HALF + lane];
}
