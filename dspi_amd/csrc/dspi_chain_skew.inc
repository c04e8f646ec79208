// dspi_chain_skew.inc — the LATENCY layout of the float chain: for launches that cannot fill the chip (BASELINE config 2: 4 096 streams,
// master PEQ only).  Included by dspi_kernels.hip after dspi_chain_pk.inc (same namespace, same helpers).
//
// Why: a stream's EQ cascade is a recurrence in time AND a chain in the band index (dsp_pipeline.c:281-365: band b+1 of frame n needs
// band b of frame n and band b+1 of frame n-1).  The packed kernel walks it band-major in 16-frame chunks, which puts a whole band's
// state recurrence (16 dependent steps) on the critical path ten times per chunk: a launch lasts steps x step time whatever the lanes
// hold, 52.7 ms for config 2's 2 000 packets.  Here the cascade is SKEWED across lanes (tools/probe/probe8.hip, traversal B): one lane
// per (channel, stage), stage s works on frame t - s while stage s+1 works on frame t - s - 1, the sample moves one lane up per step
// through a DPP row shift.  One band-sample of dependent arithmetic per frame is left on the critical path, whatever the band count
// and whatever the mix of band forms (they sit in different lanes).  Every (band, frame) node does the same IEEE operations in the same
// order as the reference, so the result is bit-identical — only the traversal order of the (band, frame) grid differs.
//
// Shape: a lane carries TWO streams (the packed layout's stream pair, same parameter image) as the halves of v2f values; a 16-lane row
// is one channel (left / right) of a stream pair: stages 0-1 the loudness shelves (usb_audio.c:688-718), 2-11 the master EQ bands
// (:721-728), 12 the crossfeed low-pass + the master peak meter (crossfeed.c:137-138, usb_audio.c:741-749), 13 the crossfeed all-pass
// (:145-148), 14 the cross-channel sum (:150-153, the partner row's all-pass output comes across the wave).  A workgroup = 8 stream
// pairs = 16 rows = four SYSTOLIC waves, plus four OUTPUT waves.  Time is cut into batches of whole packets (as many as fit 192
// frames): the systolic waves convert + preamp the batch's input into LDS (one lane per frame; the words were requested a batch
// ahead) and run its steps — stage 0 reads LDS, stage 14 writes LDS —, while the output waves work on the batch before: matrix mix,
// gain, delay line, peaks, words, one lane per frame, so a stream's S/PDIF pair buffer is written as whole coalesced lines.  One
// barrier per batch; the post-crossfeed rows are double-buffered.
//
// Scope (dspi_plan.cpp skew_class / skew_pair_limit): float lanes in launches small enough to leave the chip underfilled.  A workgroup runs
// one parameter image; a lane whose two streams carry different images runs in two workgroups, once per image, with the other half
// inactive (sk_ha / sk_hb: every store is per half) — so any assignment of presets to streams is served.  Three shapes by the image's class: no output runs an EQ (this file, EQO = false: the output side is
// frame-parallel), outputs with EQs (this file, EQO = true: every output a systolic row), leveller on (dspi_chain_skew_lev.inc).  Same
// state arrays, delay lines, rings and image as every other kernel: a context may change kernels between two calls.
template <int K> struct SkC { static constexpr int value = K; };
// Two shapes of the workgroup (eight waves either way):
//   EQO = false  no output runs an EQ: 8 stream pairs, 16 master rows on four systolic waves, four frame-parallel output waves which mix
//                the post-crossfeed samples themselves (BASELINE config 2's class);
//   EQO = true   outputs with EQ: 2 stream pairs, 4 master rows on one wave, 18 OUTPUT ROWS (pair x output: stage 0 the matrix mix, stages
//                1-10 the output's bands, stage 11 hands the sample on) on five more systolic waves a batch behind the master rows, two
//                frame-parallel output waves another batch behind (gain, delay line, meters, words).  The master rows run kSkOutDepth
//                frames further ahead, so that what the output rows emit is again a batch of whole packets.
template <bool EQO> struct SkCfg {
    static constexpr int pairs = EQO ? 2 : 8;                       // stream pairs per workgroup
    static constexpr int mrows = 2 * pairs;                         // master rows (pair x channel)
    static constexpr int mwaves = mrows / 4;
    static constexpr int orows = EQO ? 9 * pairs : 0;               // output rows
    static constexpr int owaves = (orows + 3) / 4;
    static constexpr int emit_waves = EQO ? 2 : 4, emit_pairs = pairs / emit_waves;
    static constexpr int waves = mwaves + owaves + emit_waves;
    static constexpr int ex = EQO ? 11 : 0;                         // extra lead of the master rows = depth of an output row
};
static_assert(SkCfg<false>::waves == 8 && SkCfg<true>::waves == 8, "one block size");
constexpr int kSkWaves = 8;
constexpr int kSkDepth = 14;           // stage 14 finishes frame t - 14 in step t
constexpr int kSkOutDepth = 11;        // an output row's stage 11 hands on frame t - 11 in step t
constexpr int kSkMaxB = 192;           // DSPI_MAX_BLOCK_LEN
constexpr int kSkMaxG = 8;             // packets per batch at most
constexpr int kSkPeakSlots = 64;       // packets whose master peak is posted before their output phase has run (>= 2 G + depth / B + 2)

// lane i takes lane i-1's value inside its 16-lane row (row_shr:1); lane 0 of a row, which has no source lane, keeps `edge`.
// Inline assembly on purpose: with the builtin (__builtin_amdgcn_update_dpp with a live `old` operand) on the two halves of a v2f the
// compiler emitted ONE v_mov_b32_dpp and copied its result into the second half (hipcc 7.2, seen in the ISA; ds_swizzle below likewise).
// The s_nop covers the two wait states a DPP read needs after a VALU write of its source, which the compiler cannot see in here.
__device__ __forceinline__ float sk_shr1f(float v, float edge) {
    float r = edge;
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ v2f sk_shr1(v2f v, v2f edge) { return v2f{sk_shr1f(v.x, edge.x), sk_shr1f(v.y, edge.y)}; }
// ... both halves in one statement, the result in the edge's own registers (the steady step: one s_nop for the pair, no copy of the edge)
__device__ __forceinline__ void sk_shr1_into(v2f &edge_io, v2f v) {
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %3 row_shr:1 row_mask:0xf bank_mask:0xf"
                 : "+v"(edge_io.x), "+v"(edge_io.y) : "v"(v.x), "v"(v.y));
}
// an 8-byte LDS store by the lanes of `mask` only, the wave's EXEC being full before and after (the steady step's stage-14 store: three
// instructions, no branch; the compiler's own masked store is s_and_saveexec + two branches + s_or)
__device__ __forceinline__ void sk_lds_store_masked(uint32_t lds_addr, v2f v, unsigned long long mask) {
    asm volatile("s_mov_b64 exec, %2\n\tds_write_b64 %0, %1\n\ts_mov_b64 exec, -1" :: "v"(lds_addr), "v"(v), "s"(mask) : "memory");
}
__device__ __forceinline__ v2f sk_swap16(v2f v) {         // the same lane of the partner row (rows 2i and 2i+1 of a wave)
    // (ds_bpermute; two ds_swizzle(SWAP,16) of the halves were merged into one by the compiler — the second half got the first's value)
    return v2f{__shfl_xor(v.x, 16), __shfl_xor(v.y, 16)};
}
// Which halves of a lane's stream pair take part in the launch (low 16 bits: first streams, high 16: second streams, bit = pair of the
// workgroup).  A half that does not — the second stream of a context's last lane, or the stream of another preset, which runs as a pair
// of its own in another workgroup — is computed along (on the other half's coefficients) and never stored: every store below is per half.
__device__ __forceinline__ bool sk_ha(uint32_t hm, uint32_t pi) { return (hm >> pi) & 1u; }
__device__ __forceinline__ bool sk_hb(uint32_t hm, uint32_t pi) { return (hm >> (16u + pi)) & 1u; }
__device__ __forceinline__ void sk_st2(uint32_t *p, v2u v, bool ha, bool hb) {
    if (ha && hb) *reinterpret_cast<v2u *>(p) = v;
    else if (ha) p[0] = v.x;
    else if (hb) p[1] = v.y;
}
__device__ __forceinline__ v2f sk_peak(v2f pk, v2f x) { return v2f{peak_acc(pk.x, x.x), peak_acc(pk.y, x.y)}; }      // max(pk, |x|), one instruction per half
// maximum of a non-negative value over the wave (DPP scan inside the rows, then across them), returned to every lane
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float sk_dppmax(float v) {
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ float sk_wave_max(float v) {
    v = sk_dppmax<0x111, 0xf>(v); v = sk_dppmax<0x112, 0xf>(v); v = sk_dppmax<0x114, 0xf>(v); v = sk_dppmax<0x118, 0xf>(v);      // row_shr 1 2 4 8
    v = sk_dppmax<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = sk_dppmax<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- paired presets (PP): the stream slots of a workgroup hold DIFFERENT parameter images of ONE structure (dspi_plan.h ImageSig: what
// steers control flow — flags, band forms, bypasses, enables, the crosspoints' zero pattern, delays in samples, rate — is equal), the case
// of a small context in which every stream has a preset of its own.  Structural reads keep coming from the item's image; every NUMBER
// (band coefficients, preamps, volumes, crosspoint and output gains, the leveller's and the crossfeed's constants) becomes a
// v2f {first stream's image, second stream's image} of the lane's pair: the packed operations take it as they take a splat, so the two
// halves of a lane and the pairs of a workgroup serve four (shapes 2, 3) or sixteen (shape 1) presets where they served one.
template <bool PP> struct SkNum { typedef float type; };
template <> struct SkNum<true> { typedef v2f type; };
struct SkPairImg { const DevImage *a, *b; };
// the images of the two streams in columns col, col + 1 of row wg (a half that takes no part in the launch — hm — keeps the item's image)
template <bool PP>
__device__ __forceinline__ SkPairImg sk_pair_img(const KArgs &a, const DevImage *im, uint32_t wg, uint32_t col, bool ha, bool hb) {
    SkPairImg p{im, im};
    if (PP) {
        const uint32_t s = wg * ROWP + col;
        if (ha) p.a = a.img + a.stream_image[s];
        if (hb) p.b = a.img + a.stream_image[s + 1u];
    }
    return p;
}
template <bool PP, class G> __device__ __forceinline__ typename SkNum<PP>::type sk_num(const SkPairImg &p, G get) {
    if constexpr (PP) return v2f{get(p.a), get(p.b)};
    else return get(p.a);
}
__device__ __forceinline__ float sk_half(float v, int) { return v; }
__device__ __forceinline__ float sk_half(v2f v, int c) { return v[c]; }
// the six numbers of band `bd` of the item's image `im`, from the pair's images (the band sits at the same offset in each)
template <bool PP, class NT>
__device__ __forceinline__ void sk_band_nums(const SkPairImg &p, const DevImage *im, const DevBand *bd, NT &c0, NT &c1, NT &c2, NT &c3, NT &c4, NT &c5) {
    const size_t off = (size_t)(reinterpret_cast<const char *>(bd) - reinterpret_cast<const char *>(im));
    auto at = [&](int k) { return sk_num<PP>(p, [&](const DevImage *q) { return reinterpret_cast<const DevBand *>(reinterpret_cast<const char *>(q) + off)->c[k].f; }); };
    c0 = at(0); c1 = at(1); c2 = at(2); c3 = at(3); c4 = at(4); c5 = at(5);
}

// one band-sample of both streams, the form of this lane's band (dsp_pipeline.c:298-362; band_loop_f32 above, same statements)
template <bool FMA, class NT>
__device__ __forceinline__ v2f sk_band(uint32_t kind, v2f in, v2f &s1, v2f &s2, NT c0, NT c1, NT c2, NT c3, NT c4, NT c5) {
    if (kind == K_BYPASS) return in;
    if (kind == K_BIQUAD) {
        const v2f y = mad2<FMA>(c0, in, s1);
        s1 = mad2<FMA>(c1, in, -(c3 * y)) + s2;
        s2 = mad2<FMA>(c2, in, -(c4 * y));
        return y;
    }
    const v2f v3 = in - s2;
    const v2f v1 = mad2<FMA>(c0, s1, c1 * v3);
    const v2f v2 = mad2<FMA>(c2, v3, mad2<FMA>(c1, s1, s2));
    s1 = mad2<FMA>(2.0f, v1, -s1);
    s2 = mad2<FMA>(2.0f, v2, -s2);
    if (kind == K_SVF_LP) return v2;
    if (kind == K_SVF_HP) return mad2<FMA>(c3, v1, in) - v2;
    if (kind == K_SVF_PK) return mad2<FMA>(c3, v1, in);
    return mad2<FMA>(c5, v2, mad2<FMA>(c3, in, c4 * v1));
}

template <bool EQO> struct SkShared {
    typedef SkCfg<EQO> C;
    v2f xin[C::mrows][kSkMaxB + 1];        // the batch's converted input, per row: {stream a, stream b} (+ 1: the steady loop reads one ahead)
    v2f xout[2][C::mrows][kSkMaxB + 1];    // post-crossfeed samples of a batch, double-buffered between the wave groups (+ 1: read ahead)
    v2f yout[EQO ? 2 : 1][EQO ? C::orows : 1][EQO ? kSkMaxB : 1];      // what the output rows hand on (mixed, equalised), double-buffered
    v2f mpk[kSkPeakSlots][C::mrows];       // master peak of a finished packet (stage 12 -> output waves)
    v2f dump[64 * (C::mwaves + C::owaves)];      // where the lanes that are not a row's last stage put their copy of the step's store
    v2f stage[C::emit_waves][64];                // output waves: 64 frames of one output, for delays shorter than that
};

// ---- the master rows: rows 4 w .. 4 w + 3 = stream pairs 2 w, 2 w + 1 ----
template <bool FMA, bool PCM24, bool EQO, bool PP>
__device__ __forceinline__ void sk_systolic(const KArgs &a, SkShared<EQO> &sh, ImgPtr img, const DevImage *im, uint32_t wg, uint32_t part, uint32_t pmask, uint32_t hm, int wave, uint32_t lane) {
    typedef SkCfg<EQO> C;
    constexpr int kSkPairs = C::pairs;
    constexpr uint32_t kLead = (uint32_t)(kSkDepth + C::ex);      // frames stage 0 is ahead of the batch's first packet
    constexpr StateMap sm = make_state_map(1);
    const uint32_t flags = img->flags;
    const uint32_t B = a.block_len, n_blocks = a.n_blocks, total = n_blocks * B;
    const size_t F = total;
    uint32_t *gs0 = a.state + (size_t)wg * sm.n_slots * ROWP;
    const uint32_t row = (uint32_t)wave * 4u + (lane >> 4), l = lane & 15u;
    const uint32_t pi = row >> 1, ch = row & 1u;
    const bool row_live = (pmask >> pi) & 1u;
    const uint32_t col = (part * kSkPairs + pi) * 2u;            // the pair's first column in every [..][128] array
    const bool xf_on = flags & IF_CROSSFEED_ON;
    typedef typename SkNum<PP>::type NT;                          // a number of the preset: one for the lane's two streams, or one each (PP)
    const SkPairImg pim = sk_pair_img<PP>(a, im, wg, col, sk_ha(hm, pi), sk_hb(hm, pi));
    uint32_t kind = K_BYPASS;
    NT c0 = NT(0.0f), c1 = NT(0.0f), c2 = NT(0.0f), c3 = NT(0.0f), c4 = NT(0.0f), c5 = NT(0.0f);
    v2f s1 = splat(0.0f), s2 = splat(0.0f);
    int slot1 = -1, slot2 = -1;                                  // where the stage's state lives ([slot][128])
    {
        const DevBand *bd = nullptr;                             // per-lane loads (a stage's band differs from lane to lane)
        if (l < 2) { bd = &im->loud[l]; slot1 = sm.loud + (int)((ch * 2u + l) * 2u); slot2 = slot1 + 1; }
        else if (l < 12) {
            const bool on = !(flags & IF_BYPASS_MASTER_EQ) && !((img->ch_bypassed >> ch) & 1u);      // usb_audio.c:721-728
            if (on) bd = &im->eq[ch][l - 2];
            slot1 = sm.eq + (int)((ch * kBands + (l - 2)) * 2u); slot2 = slot1 + 1;
        } else if (l == 12) {
            c0 = sk_num<PP>(pim, [](const DevImage *q) { return q->xf_lp_a0.f; }); c1 = sk_num<PP>(pim, [](const DevImage *q) { return q->xf_lp_b1.f; });
            slot1 = sm.xfeed + (int)ch;
        } else if (l == 13) { c0 = sk_num<PP>(pim, [](const DevImage *q) { return q->xf_ap_a.f; }); slot1 = sm.xfeed + 2 + (int)ch; }
        if (bd) { kind = bd->kind; sk_band_nums<PP>(pim, im, bd, c0, c1, c2, c3, c4, c5); }
        if (row_live) {
            if (slot1 >= 0) s1 = as_v2f(*reinterpret_cast<const v2u *>(gs0 + (size_t)slot1 * ROWP + col));
            if (slot2 >= 0) s2 = as_v2f(*reinterpret_cast<const v2u *>(gs0 + (size_t)slot2 * ROWP + col));
        }
    }
    // Every form keeps its own state registers, every lane updates all of them in the steady-state loop below (no selects, no branches);
    // only the registers of the lane's own form hold meaning, and those are what goes back to the state array.
    const bool is_bq = kind == K_BIQUAD, is_lp = kind == K_SVF_LP, is_hp = kind == K_SVF_HP, is_pk = kind == K_SVF_PK, is_sh = kind == K_SVF_SHELF;
    const bool is12 = l == 12, is14 = l == 14;
    const bool any_bq = __any(is_bq), any_oth = __any(is_lp || is_hp || is_sh), any_pk = __any(is_pk);      // wave-uniform
    v2f sq1 = s1, sq2 = s2, xs = s1;                             // biquad s1 s2 | (s1, s2 themselves: the SVF's ic1eq ic2eq) | crossfeed lp (stage 12) / all-pass (13)
    v2f o0 = splat(0.0f), o1 = splat(0.0f), o2 = splat(0.0f);   // what the stage hands up: sample | + low-pass | + all-pass
    v2f pk = splat(0.0f);
    uint32_t fp = 0, kp = 0;                                     // stage 12: position inside the packet, packet index
    uint32_t t = 0;                                              // global step = the frame stage 0 reads
    // input scale x preamp of the wave's two pairs (usb_audio.c:591-686)
    NT gl_in[2], gr_in[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t p = 2u * (uint32_t)wave + (uint32_t)h;
        const SkPairImg ph = sk_pair_img<PP>(a, im, wg, (part * kSkPairs + p) * 2u, sk_ha(hm, p), sk_hb(hm, p));
        gl_in[h] = (PCM24 ? 1.0f / 8388608.0f : 1.0f / 32768.0f) * sk_num<PP>(ph, [](const DevImage *q) { return q->preamp[0].f; });
        gr_in[h] = (PCM24 ? 1.0f / 8388608.0f : 1.0f / 32768.0f) * sk_num<PP>(ph, [](const DevImage *q) { return q->preamp[1].f; });
    }

    // the next batch's input words are requested a batch ahead (16-bit input): registers for the wave's own two pairs, both streams
    constexpr int kRawG = (kSkMaxB + 63) / 64;
    uint32_t raw[2][2][kRawG];
    const uint32_t G = min((uint32_t)kSkMaxG, B >= (uint32_t)kSkMaxB ? 1u : (uint32_t)kSkMaxB / B);
    auto window = [&](int p0_, uint32_t &ws_, uint32_t &len_) {      // batch "-1" = the pipeline fill: the first kSkDepth frames enter, nothing leaves yet
        ws_ = p0_ < 0 ? 0u : (uint32_t)p0_ * B + kLead;
        len_ = p0_ < 0 ? kLead : (min((uint32_t)p0_ + G, n_blocks) - (uint32_t)p0_) * B;
    };
    auto load_raw = [&](int p0_) {
        uint32_t ws_, len_; window(p0_, ws_, len_);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t p = 2u * (uint32_t)wave + h, stream = wg * ROWP + (part * kSkPairs + p) * 2u;
            const bool live = (pmask >> p) & 1u;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int g_ = 0; g_ < kRawG; ++g_) {
                    const uint32_t j = (uint32_t)g_ * 64u + lane, f = ws_ + j;
                    raw[h][c][g_] = 0u;
                    if (live && j < len_ && f < total && (c ? sk_hb(hm, p) : sk_ha(hm, p))) raw[h][c][g_] = static_cast<const uint32_t *>(a.pcm)[(size_t)(stream + c) * F + f];
                }
        }
    };
    if (!PCM24) load_raw(-1);

    uint32_t buf = 0;
    // (a wave neither of whose pairs takes part in the launch — a workgroup that holds a stream or two — only passes the barriers: its
    //  arithmetic would take issue slots from the wave it shares a SIMD with)
    const bool wave_live = ((pmask >> (2u * (uint32_t)wave)) & 3u) != 0u;
    for (int p0 = -1; p0 < (int)n_blocks; p0 = p0 < 0 ? 0 : p0 + (int)G) {
        if (!wave_live) { __syncthreads(); if (p0 >= 0 || EQO) buf ^= 1u; continue; }
        uint32_t ws, len;
        window(p0, ws, len);           // ws: first frame stage 0 reads in this batch
        const int p_next = p0 < 0 ? 0 : p0 + (int)G;
        // ---- input conversion + preamp (usb_audio.c:591-686), one lane per frame; the wave's own rows: no barrier before the steps ----
        if (!PCM24) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t p = 2u * (uint32_t)wave + h;
#pragma unroll
                for (int g_ = 0; g_ < kRawG; ++g_) {
                    const uint32_t j = (uint32_t)g_ * 64u + lane;
                    if (j < len) {
                        const uint32_t wa = raw[h][0][g_], wb = raw[h][1][g_];
                        sh.xin[2 * p][j] = v2f{(float)(int32_t)(int16_t)(wa & 0xffffu), (float)(int32_t)(int16_t)(wb & 0xffffu)} * gl_in[h];
                        sh.xin[2 * p + 1][j] = v2f{(float)((int32_t)wa >> 16), (float)((int32_t)wb >> 16)} * gr_in[h];
                    }
                }
            }
            if (p_next < (int)n_blocks) load_raw(p_next);          // lands under the steps below
        } else {
            for (uint32_t h = 0; h < 2u; ++h) {
                const uint32_t p = 2u * (uint32_t)wave + h;
                const bool live = (pmask >> p) & 1u;
                const uint32_t stream = wg * ROWP + (part * kSkPairs + p) * 2u;
                for (uint32_t j = lane; j < len; j += 64u) {
                    const uint32_t f = ws + j;
                    v2f xl = splat(0.0f), xr = splat(0.0f);
                    if (live && f < total) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            if (!(c ? sk_hb(hm, p) : sk_ha(hm, p))) continue;
                            const uint16_t *q = reinterpret_cast<const uint16_t *>(static_cast<const uint8_t *>(a.pcm) + ((size_t)(stream + c) * F + f) * 6);
                            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                            xl[c] = (float)((int32_t)((w0 | (w1 << 16)) << 8) >> 8);
                            xr[c] = (float)((int32_t)(((w1 >> 8) | (w2 << 8)) << 8) >> 8);
                        }
                    }
                    sh.xin[2 * p][j] = xl * (h ? gl_in[1] : gl_in[0]);
                    sh.xin[2 * p + 1][j] = xr * (h ? gr_in[1] : gr_in[0]);
                }
            }
        }
        // (the rows just written are this wave's own: LDS works through a wave's instructions in program order)
        // ---- systolic steps ----
        v2f nx = sh.xin[row][0];
        v2f (*xo)[kSkMaxB + 1] = sh.xout[buf];
        // Steady steps: every stage has a frame, i.e. stage 0's frame lies inside the launch — all of a batch but the launch's last one, of
        // which the first total - ws steps are (a launch of ONE packet used to run entirely on the guarded loop below).
        const uint32_t len_s = (p0 >= 0 && B >= 3u + (uint32_t)C::ex && ws < total) ? min(len, total - ws) : 0u;
        if (len_s) {
            // Straight-line step, specialised on which band forms occur in this wave (wave-uniform) and on the crossfeed: every lane
            // computes those forms and keeps the one of its own band; stage 14's store goes to LDS for every lane (the others hit a
            // scratch slot) and leaves at the top of the NEXT step, ahead of that step's read (LDS returns in order: the wait for the
            // read then never waits for a store issued a moment ago); stage 12 ends a packet in step B - 3 (- the extra lead) of it.
            // (round 6: only the four stage-14 lanes store — an EXEC-masked 8-byte write, one LDS cycle — instead of all 64 with 60 of them aimed at a
            //  dump slot: the dump writes were the kernel's LDS bank conflicts, SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_LDS 0.86 in profiles/r05l,
            //  0 in profiles/r06l; config 2 12.28 -> 12.09 ms on one box)
            // (round 6, second pass: the lone systolic wave of a SIMD issues one instruction per ~5 cycles whatever it is, so the step is its
            //  instruction COUNT — 52 for config 2.  Hand-tuned: the stage-14 store is three instructions of inline assembly (EXEC := the four
            //  lanes, ds_write_b64, EXEC := all) instead of a saveexec / branch / branch / restore sequence; the two DPP moves share one s_nop and
            //  write into the edge value's own registers; the step is written twice per iteration so that the input sample read one step ahead
            //  needs no copy at the loop's back edge.  No arithmetic is touched.)
            const uint32_t wrow_addr = (uint32_t)(uintptr_t)&xo[row][0];      // (a generic pointer to LDS: its low word is the LDS address)
            const unsigned long long m14 = __ballot(is14);
            auto run = [&](auto bq_, auto pk_, auto oth_, auto xf_) {
                constexpr bool BQ = decltype(bq_)::value != 0, PKF = decltype(pk_)::value != 0, OTH = decltype(oth_)::value != 0, XF = decltype(xf_)::value != 0;
                uint32_t pkt = (uint32_t)p0;                         // the packet stage 12 is finishing
                uint32_t left = B - 2u - (uint32_t)C::ex;            // steps until stage 12 ends a packet: in step B - 3 (- the extra lead) of it, then every B steps (one counter: three scalar instructions per step instead of five)
                // one step: `x` comes in holding the batch's input sample of this frame (lane 0's edge) and leaves as this lane's input
                auto step = [&](uint32_t j, v2f x) {
                    sk_shr1_into(x, o0);                             // stage 0 keeps the batch's input, every other stage takes its neighbour's output
                    v2f out = x;
                    if (PKF || OTH) {                                // Cytomic SVF core (dsp_pipeline.c:298-343), then the form's output
                        const v2f v3 = x - s2;
                        const v2f v1 = mad2<FMA>(c0, s1, c1 * v3);
                        const v2f v2 = mad2<FMA>(c2, v3, mad2<FMA>(c1, s1, s2));
                        s1 = mad2<FMA>(2.0f, v1, -s1);
                        s2 = mad2<FMA>(2.0f, v2, -s2);
                        const v2f A = mad2<FMA>(c3, v1, x);
                        if (PKF) out = is_pk ? A : out;
                        if (OTH) {
                            out = is_lp ? v2 : out;
                            out = is_hp ? A - v2 : out;
                            out = is_sh ? mad2<FMA>(c5, v2, mad2<FMA>(c3, x, c4 * v1)) : out;
                        }
                    }
                    if (BQ) {                                        // TDF2 biquad (:347-362)
                        const v2f y = mad2<FMA>(c0, x, sq1);
                        sq1 = mad2<FMA>(c1, x, -(c3 * y)) + sq2;
                        sq2 = mad2<FMA>(c2, x, -(c4 * y));
                        out = is_bq ? y : out;
                    }
                    pk = sk_peak(pk, x);
                    v2f res = x;
                    if (XF) {                                        // crossfeed.c:137-153, stages 12 / 13 / 14
                        const v2f p1 = sk_shr1(o1, splat(0.0f));
                        const v2f other = sk_swap16(sk_shr1(o2, splat(0.0f)));
                        const v2f lp = mad2<FMA>(c0, x, c1 * xs);
                        const v2f ap = mad2<FMA>(c0, p1, xs);
                        const v2f aps = mad2<FMA>(-c0, ap, p1);
                        xs = is12 ? lp : aps;
                        o1 = is12 ? lp : p1;
                        o2 = ap;
                        res = (x - p1) + other;
                    }
                    o0 = out;
                    // stage 14's sample of this step goes to the batch's row now (the next read of the input row is waited for ~40 instructions
                    // later: LDS returns in order, and by then this store has long left)
                    sk_lds_store_masked(wrow_addr + j * (uint32_t)sizeof(v2f), res, m14);
                    if (--left == 0u) {
                        if (is12) sh.mpk[pkt & (kSkPeakSlots - 1)][row] = pk;
                        pk = splat(0.0f);
                        ++pkt;
                        left = B;
                    }
                };
                uint32_t j = 0;
                v2f na = nx, nb;                                     // the input samples of steps j and j + 1 (the row has a spare element)
                for (; j + 2u <= len_s; j += 2u) {
                    nb = sh.xin[row][j + 1];
                    step(j, na);
                    na = sh.xin[row][j + 2];
                    step(j + 1u, nb);
                }
                if (j < len_s) { nb = sh.xin[row][j + 1]; step(j, na); na = nb; ++j; }
                nx = na;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the assembly's stores are not in the compiler's count: they have left before the barrier below)
            };
            auto run_x = [&](auto bq_, auto pk_, auto oth_) { if (xf_on) run(bq_, pk_, oth_, SkC<1>{}); else run(bq_, pk_, oth_, SkC<0>{}); };
            auto run_o = [&](auto bq_, auto pk_) { if (any_oth) run_x(bq_, pk_, SkC<1>{}); else run_x(bq_, pk_, SkC<0>{}); };
            auto run_p = [&](auto bq_) { if (any_pk) run_o(bq_, SkC<1>{}); else run_o(bq_, SkC<0>{}); };
            if (any_bq) run_p(SkC<1>{}); else run_p(SkC<0>{});
            t += len_s;
            kp += (fp + len_s) / B; fp = (fp + len_s) % B;      // where stage 12 stands (it began the batch 2 + ex frames into packet p0)
        }
        {
            // fill, drain and packets shorter than three frames: a stage may have no frame in a step, the roles branch
#pragma unroll 1
            for (uint32_t j = len_s; j < len; ++j) {
                const v2f x0 = nx;
                nx = sh.xin[row][j + 1];
                const v2f x = sk_shr1(o0, x0);
                v2f p1 = splat(0.0f), other = splat(0.0f);
                if (xf_on) {
                    p1 = sk_shr1(o1, splat(0.0f));
                    other = sk_swap16(sk_shr1(o2, splat(0.0f)));  // stage 14: the partner channel's all-pass output of the same frame
                }
                const bool act = t >= l && t - l < total;            // this stage has a frame in this step
                if (act) {
                    if (l < 12) o0 = is_bq ? sk_band<FMA>(kind, x, sq1, sq2, c0, c1, c2, c3, c4, c5) : sk_band<FMA>(kind, x, s1, s2, c0, c1, c2, c3, c4, c5);
                    else if (l == 12) {
                        if (fp == 0) pk = splat(0.0f);
                        pk = sk_peak(pk, x);                         // master peaks, before the crossfeed (usb_audio.c:741-749)
                        if (fp + 1 == B) { sh.mpk[kp & (kSkPeakSlots - 1)][row] = pk; fp = 0; ++kp; } else ++fp;
                        o0 = x;
                        if (xf_on) { const v2f lp = mad2<FMA>(c0, x, c1 * xs); xs = lp; o1 = lp; }          // crossfeed.c:137-138
                    } else if (l == 13) {
                        o0 = x;
                        if (xf_on) { const v2f ap = mad2<FMA>(c0, p1, xs); xs = mad2<FMA>(-c0, ap, p1); o1 = p1; o2 = ap; }      // :145-148
                    } else if (l == 14) {
                        xo[row][j] = xf_on ? (x - p1) + other : x;                                         // :150-153
                    }
                }
                ++t;
            }
        }
        __syncthreads();               // the batch's rows are complete; the output waves are done with the other buffer
        if (p0 >= 0 || EQO) buf ^= 1u; // (output rows: the fill's first frames are their fill)
    }
    __syncthreads();                   // (the output waves' last batch)
    if (EQO) __syncthreads();          // (... which is two batches behind when output rows sit in between)
    // ---- state back ----
    if (row_live) {
        const v2f e1 = l >= 12 ? xs : (is_bq ? sq1 : s1), e2 = is_bq ? sq2 : s2;
        const bool idle = l < 12 && kind == K_BYPASS;      // (a bypassed band's state is left alone, as the reference leaves it — dsp_pipeline.c:288-289; the steady loop's state registers of such a lane hold no meaning: with zero coefficients s1 changes sign every step)
        if (slot1 >= 0 && !idle) sk_st2(gs0 + (size_t)slot1 * ROWP + col, as_v2u(e1), sk_ha(hm, pi), sk_hb(hm, pi));
        if (slot2 >= 0 && !idle) sk_st2(gs0 + (size_t)slot2 * ROWP + col, as_v2u(e2), sk_ha(hm, pi), sk_hb(hm, pi));
    }
}

// ---- the output waves (usb_audio.c:753-959), one lane per frame; wave w serves pairs w and w + 4, a batch behind the systolic waves ----
template <bool FMA, bool EQO, bool SPDIF, bool PP>
__device__ __forceinline__ void sk_outputs(const KArgs &a, SkShared<EQO> &sh, ImgPtr img, const DevImage *im, uint32_t wg, uint32_t part, uint32_t pmask, uint32_t hm, int ow, uint32_t lane) {
    typedef SkCfg<EQO> C;
    constexpr int kSkPairs = C::pairs, kPer = C::emit_pairs;      // pairs per workgroup, pairs per output wave (pairs ow, ow + emit_waves, ...)
    constexpr StateMap sm = make_state_map(1);
    constexpr int N = sm.n_out, P = sm.n_pairs;
    const uint32_t flags = img->flags;
    const uint32_t B = a.block_len, n_blocks = a.n_blocks;
    const size_t F = (size_t)n_blocks * B;
    uint32_t *gs0 = a.state + (size_t)wg * sm.n_slots * ROWP;
    // channel status of THIS image's sample rate (audio_spdif.c:250-256): a context may hold streams at different rates
    [[maybe_unused]] const uint32_t sp_lo = spdif_status_lo(img->fs_hz);
    // Output rows (two pairs, two output waves) and ONE pair in the launch (a context of a stream or two): the two waves share its outputs —
    // wave 0 the first two S/PDIF pairs and the master meters, wave 1 the other two and the sub — instead of one of them idling; both carry
    // the pair's packet scalars (the same arithmetic on the same state), wave 0 writes them back.
    const bool split = EQO && (pmask & (pmask - 1u)) == 0u;
    const uint32_t lp = (pmask & 1u) ? 0u : 1u;
    auto pr_mine = [&](int pr) { return !split || ((pr < 2) == (ow == 0)); };
    const bool ch_mine = !split || ((lane < 6u) == (ow == 0));      // meter words: lanes 0-1 the master channels, 2 + o the outputs
    struct OutSt { v2u widx, loading, counter, clip, rpos; v2f smooth, vmm; };
    OutSt os[kPer];
    bool ow_live[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
        const uint32_t opi = (split ? lp : (uint32_t)ow + (uint32_t)C::emit_waves * h), ocol = (part * kSkPairs + opi) * 2u;
        ow_live[h] = (pmask >> opi) & 1u;
        os[h].widx = os[h].loading = os[h].counter = os[h].clip = os[h].rpos = v2u{0u, 0u};
        os[h].smooth = os[h].vmm = splat(0.0f);
        if (ow_live[h]) {
            os[h].widx = *reinterpret_cast<const v2u *>(gs0 + (size_t)sm.widx * ROWP + ocol);
            os[h].loading = *reinterpret_cast<const v2u *>(gs0 + (size_t)(sm.mute + 0) * ROWP + ocol);
            os[h].counter = *reinterpret_cast<const v2u *>(gs0 + (size_t)(sm.mute + 1) * ROWP + ocol);
            os[h].smooth = as_v2f(*reinterpret_cast<const v2u *>(gs0 + (size_t)(sm.mute + 2) * ROWP + ocol));
            os[h].rpos = *reinterpret_cast<const v2u *>(gs0 + (size_t)sm.ring_pos * ROWP + ocol);
        }
    }
    typedef typename SkNum<PP>::type NT;
    const float vol_f = img->vol.f, master_f = img->master.f;
    const uint32_t mute_transition = img->mute_transition;
    // launch-invariant parameters of the outputs (wave-uniform: scalar registers), read once
    struct OutC { bool enabled, muted, gl_nz, gr_nz, dl_on, metered, work; float gl, gr, og; int32_t dly; };
    OutC oc[N];
    float word_scale[P];
    const bool sub_active = flags & IF_SUB_ACTIVE;
#pragma unroll
    for (int o = 0; o < N; ++o) {
        const bool is_sub = o == N - 1, processed = !is_sub || sub_active;
        oc[o].enabled = (img->out_enabled >> o) & 1u; oc[o].muted = (img->out_mute >> o) & 1u;
        oc[o].gl = img->mix[0][o].f; oc[o].gr = img->mix[1][o].f; oc[o].gl_nz = oc[o].gl != 0.0f; oc[o].gr_nz = oc[o].gr != 0.0f;
        oc[o].og = img->out_gain_lin[o]; oc[o].dly = img->delay_samples[o];
        oc[o].dl_on = processed && (flags & IF_ANY_DELAY) && oc[o].dly > 0;
        oc[o].metered = !is_sub || (sub_active && oc[o].enabled);
        oc[o].work = oc[o].enabled || oc[o].dl_on;      // otherwise the output is digital silence: zero words, zero peak
    }
#pragma unroll
    for (int pr = 0; pr < P; ++pr) word_scale[pr] = (oc[2 * pr].enabled || oc[2 * pr + 1].enabled) ? 8388607.0f : 0.0f;      // usb_audio.c:930-933
    // The line of a disabled sub (round 6).  The reference runs an output's delay line whenever its delay is non-zero, enabled or not
    // (usb_audio.c:898-911), and the sub always carries its alignment delay (config.h:93-95) — so BASELINE config 2, which enables two
    // outputs, still writes the sub's zeros into its line and reads them back: four scattered 4-byte loads and four stores per output wave
    // and packet (exactly the kernel's surplus of VMEM instructions over its input and word traffic, and the 12 B/frame its counters showed
    // above the 12.5 of I/O: profiles/r06_config2.md), two memory round trips per pair and packet on waves with little else to wait for.
    // Without that line the kernel is 5.5 % (config 2) / 16 % (config 2b) faster.  So: a launch at least as long as the line first LOOKS at the
    // line of its pairs' streams (4 096 rows once per launch, 4 % of what the packets would read); if every word is zero — the sub has been off
    // for a line's length, or since the context was made — the disabled sub writes zeros over zeros and reads zeros: words, meters and the line
    // itself are what they would be with the traffic, and the traffic is dropped for the launch.  (A general batch-level prefetch of such lines
    // was built first and measured slower, 12.1 -> 13.1 ms: same round trips, in a burst.)  Output rows (EQO) keep the packet path.
    if (!EQO && oc[N - 1].dl_on && !oc[N - 1].enabled && F >= (size_t)sm.max_delay) {
        uint32_t acc = 0u;
#pragma unroll
        for (int h = 0; h < kPer; ++h) {
            if (!ow_live[h]) continue;
            const uint32_t opi = (uint32_t)ow + (uint32_t)C::emit_waves * h, ocol = (part * kSkPairs + opi) * 2u;
            const uint32_t *line = a.dlines + ((size_t)wg * N + (N - 1)) * (size_t)sm.max_delay * ROWP + ocol;
            for (uint32_t i = lane; i < (uint32_t)sm.max_delay; i += 64u) {
                const v2u w = *reinterpret_cast<const v2u *>(line + (size_t)i * ROWP);
                acc |= (sk_ha(hm, opi) ? w.x : 0u) | (sk_hb(hm, opi) ? w.y : 0u);
            }
        }
        if (!__any(acc != 0u)) { oc[N - 1].dl_on = false; oc[N - 1].work = oc[N - 1].enabled; }      // (wave-uniform: both pairs of the wave, or neither)
    }
    const uint32_t G = min((uint32_t)kSkMaxG, B >= (uint32_t)kSkMaxB ? 1u : (uint32_t)kSkMaxB / B);
    const uint32_t i2s_mask = a.i2s_slots ? img->i2s_pairs : 0u;
    // paired presets: the numbers among the above (crosspoint and output gains, the volumes) are those of the pair's own two images
    SkPairImg pims[kPer];
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
        const uint32_t opi = (split ? lp : (uint32_t)ow + (uint32_t)C::emit_waves * h);
        pims[h] = sk_pair_img<PP>(a, im, wg, (part * kSkPairs + opi) * 2u, sk_ha(hm, opi), sk_hb(hm, opi));
    }

    uint32_t buf = 0;
    // the same barriers as the systolic waves: one after the fill, one per batch; batch p0's rows are read while the next batch is made.
    // With output rows in between (EQO) this group is two batches behind the master rows: two more barriers first, the source is yout.
    __syncthreads();
    if (EQO) { __syncthreads(); buf = 1u; }      // (the output rows' buffers alternate from their fill on: their first batch is in buffer 0)
    for (int p0 = 0; p0 < (int)n_blocks; p0 += (int)G) {
        __syncthreads();
        const v2f (*xo)[kSkMaxB + 1] = sh.xout[EQO ? 0 : buf];
        const v2f (*yo)[EQO ? kSkMaxB : 1] = sh.yout[EQO ? (buf ^ 1u) : 0];
        buf ^= 1u;
        for (int k = p0; k < min(p0 + (int)G, (int)n_blocks); ++k) {
            const uint32_t jb = (uint32_t)(k - p0) * B;                  // the packet's first frame inside the batch rows
            const size_t frame0 = (size_t)k * B;
#pragma unroll
            for (int h = 0; h < kPer; ++h) {
                if (!ow_live[h]) continue;
                OutSt &s = os[h];
                const uint32_t opi = (split ? lp : (uint32_t)ow + (uint32_t)C::emit_waves * h), ocol = (part * kSkPairs + opi) * 2u;
                const uint32_t stream = wg * ROWP + ocol;
                const bool one = sk_ha(hm, opi), two = sk_hb(hm, opi);   // which of the lane's two streams this launch writes
                uint32_t *gs = gs0 + ocol;
                [[maybe_unused]] const SkPairImg &pim = pims[h];
                auto num_gl = [&](int o) -> NT { if constexpr (PP) return v2f{pim.a->mix[0][o].f, pim.b->mix[0][o].f}; else return oc[o].gl; };
                auto num_gr = [&](int o) -> NT { if constexpr (PP) return v2f{pim.a->mix[1][o].f, pim.b->mix[1][o].f}; else return oc[o].gr; };
                auto num_og = [&](int o) -> NT { if constexpr (PP) return v2f{pim.a->out_gain_lin[o], pim.b->out_gain_lin[o]}; else return oc[o].og; };
                {   // packet scalars, per stream: preset-mute envelope (usb_audio.c:466-498) and volumes (:564-571) — as output_item_pk
                    float step = (float)B / (float)mute_transition;
                    if (step > 1.0f) step = 1.0f;
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const bool actm = s.loading[c] != 0;
                        if (actm) {
                            if (s.counter[c] > B) s.counter[c] -= B;
                            else { s.counter[c] = 0; s.loading[c] = 0; }
                        }
                        const float target = actm ? 0.0f : 1.0f;
                        float gg = s.smooth[c];
                        if (gg < target) { gg += step; if (gg > target) gg = target; }
                        else if (gg > target) { gg -= step; if (gg < target) gg = target; }
                        s.smooth[c] = gg;
                        float vol_mul = PP ? (c ? pim.b : pim.a)->vol.f : vol_f;
                        vol_mul *= gg;
                        s.vmm[c] = vol_mul * (PP ? (c ? pim.b : pim.a)->master.f : master_f);
                    }
                }
                // the packet's meter words: lane ch collects channel ch's uint16 (stream a, stream b), one store per stream at the end
                v2u pkw = v2u{0u, 0u};
                {   // master peaks (usb_audio.c:963-966)
#pragma unroll
                    for (int mch = 0; mch < 2; ++mch) {
                        const v2f pm = sh.mpk[(uint32_t)k & (kSkPeakSlots - 1)][2 * opi + mch];
                        v2u p16;
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            p16[c] = (uint32_t)(fminf(1.0f, pm[c]) * 32767.0f);
                            if (pm[c] > 1.001f) s.clip[c] |= 1u << mch;
                        }
                        if (lane == (uint32_t)mch) pkw = p16;
                    }
                }
#pragma unroll
                for (int pr_ = 0; pr_ <= P; ++pr_) {                 // the four S/PDIF pairs, then the sub
                    const bool is_sub = pr_ == P;
                    const int o0_ = is_sub ? N - 1 : 2 * pr_, o1_ = is_sub ? N - 1 : 2 * pr_ + 1;
                    if (!pr_mine(pr_)) continue;
                    if (!oc[o0_].work && !oc[o1_].work) {
                        // silence: zero words (a pair whose two outputs are disabled is zero-filled, usb_audio.c:930-933), zero peaks;
                        // DSPI_OUT_ENABLED_ONLY: the caller does not read the buffers of silent outputs, nothing is stored
                        if (!a.skip_silent)
                        for (uint32_t j = lane; j < B; j += 64u) {
                            if (is_sub) {
                                if (a.sub) {
                                    if (a.tiled_out) sk_st2(reinterpret_cast<uint32_t *>(a.sub) + ((size_t)wg * F + frame0 + j) * ROWP + ocol, v2u{0u, 0u}, one, two);
                                    else { if (one) a.sub[(size_t)stream * F + frame0 + j] = 0; if (two) a.sub[(size_t)(stream + 1) * F + frame0 + j] = 0; }
                                }
                            } else if (a.pairs) {
                                if (a.tiled_out) {
                                    uint32_t *dst = reinterpret_cast<uint32_t *>(a.pairs) + (((size_t)wg * (N - 1) + 2 * pr_) * F + frame0 + j) * ROWP + ocol;
                                    sk_st2(dst, v2u{0u, 0u}, one, two);
                                    sk_st2(dst + F * ROWP, v2u{0u, 0u}, one, two);
                                } else if (SPDIF) {
                                    const spdif_u4 z = spdif_frame(0u, 0u, (a.spdif_pos + (uint32_t)((frame0 + j) % 192u)) % 192u, sp_lo, kSpdifStatusHi);
                                    if (one) *reinterpret_cast<spdif_u4 *>(a.pairs + (((size_t)(stream - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 4) = z;
                                    if (two) *reinterpret_cast<spdif_u4 *>(a.pairs + (((size_t)(stream + 1 - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 4) = z;
                                } else {
                                    if (one) *reinterpret_cast<v2u *>(a.pairs + (((size_t)(stream - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 2) = v2u{0u, 0u};
                                    if (two) *reinterpret_cast<v2u *>(a.pairs + (((size_t)(stream + 1 - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 2) = v2u{0u, 0u};
                                }
                            }
                        }
                        continue;
                    }
                    v2f opk[2] = {splat(0.0f), splat(0.0f)};
#pragma unroll 1
                    for (uint32_t j0 = 0; j0 < B; j0 += 64u) {
                        const uint32_t j = j0 + lane;
                        const bool fl = j < B;
                        v2f xl = splat(0.0f), xr = splat(0.0f);
                        if (!EQO) { xl = xo[2 * opi][jb + (fl ? j : 0)]; xr = xo[2 * opi + 1][jb + (fl ? j : 0)]; }
                        v2u w[2] = {v2u{0u, 0u}, v2u{0u, 0u}};
#pragma unroll
                        for (int side = 0; side < 2; ++side) {
                            if (is_sub && side) break;
                            const int o = side ? o1_ : o0_;
                            const OutC &k_ = oc[o];
                            const bool processed = !is_sub || sub_active;
                            // ---- matrix mix (usb_audio.c:753-779), the statements of output_item_pk ----
                            v2f y;
                            if (EQO) y = yo[opi * (uint32_t)N + (uint32_t)o][jb + (fl ? j : 0)];      // mixed and equalised by the output's row
                            else {
                                const bool first_l = FMA ? !k_.gr_nz : k_.gl_nz;
                                y = (first_l ? xl : xr) * (first_l ? num_gl(o) : num_gr(o));
                                if (k_.enabled && k_.gl_nz && k_.gr_nz) y = FMA ? mad2<true>(num_gl(o), xl, y) : y + xr * num_gr(o);
                                if (!k_.enabled || (!k_.gl_nz && !k_.gr_nz)) y = splat(0.0f);
                            }
                            if (processed && k_.enabled) {      // ---- gain (usb_audio.c:877-895); the EQ ran in the output's row, or is off ----
                                const v2f gain = k_.muted ? splat(0.0f) : num_og(o) * s.vmm;
                                y = y * gain;
                                if (gain.x == 0.0f) y.x = 0.0f;
                                if (gain.y == 0.0f) y.y = 0.0f;
                            }
                            if (k_.dl_on) {                     // ---- delay line (usb_audio.c:898-912): the packet's samples in, the delayed ones out ----
                                // The firmware writes sample i, then reads sample i - dly, frame after frame.  Here 64 frames at a time: the
                                // delayed sample of a frame lies (a) before these 64 frames — in the line: written by an earlier packet or an earlier
                                // group of this one (complete: the wait below), and not yet overwritten, because the line is READ BEFORE this
                                // group writes (a delay close to the maximum reads the rows just ahead of the write index: the oldest ones) —
                                // or (b) inside these 64 frames (a delay shorter than that; dly == max aliases to 0): taken from the group itself.
                                const uint32_t dmask = (uint32_t)sm.max_delay - 1u;
                                const uint32_t d_eff = (uint32_t)k_.dly & dmask;
                                uint32_t *line = a.dlines + ((size_t)wg * N + o) * (size_t)sm.max_delay * ROWP + ocol;
                                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // earlier stores of this line have landed
                                v2f yd = y;
                                if (fl) {
#pragma unroll
                                    for (int c = 0; c < 2; ++c)      // (served by L2, agent scope: not by a line this CU's L1 may hold from a revolution ago)
                                        yd[c] = as_f(__hip_atomic_load(line + (size_t)((s.widx[c] + j - (uint32_t)k_.dly) & dmask) * ROWP + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                                }
                                if (d_eff < 64u) {
                                    v2f *stage = sh.stage[ow];
                                    stage[lane] = y;
                                    if (lane >= d_eff) yd = stage[lane - d_eff];
                                }
                                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the old rows are in registers before any of them is overwritten
                                if (fl) {
#pragma unroll
                                    for (int c = 0; c < 2; ++c) if (c ? two : one) line[(size_t)((s.widx[c] + j) & dmask) * ROWP + c] = as_u(y[c]);
                                }
                                y = yd;
                            }
                            // ---- peaks, words (usb_audio.c:914-959) ----
                            if (k_.metered && fl) opk[side] = sk_peak(opk[side], y);
                            if (is_sub) {
                                const v2f z = y * 268435456.0f;
                                w[0] = (sub_active && k_.enabled) ? v2u{(uint32_t)f2i_sat(z.x), (uint32_t)f2i_sat(z.y)} : v2u{0u, 0u};
                            } else {
                                v2f d = v2f{clamp_pm1(y.x), clamp_pm1(y.y)} * word_scale[is_sub ? 0 : pr_];
                                w[side] = v2u{(uint32_t)(int32_t)d.x, (uint32_t)(int32_t)d.y};
                                if (i2s_mask & (1u << (is_sub ? 0 : pr_))) w[side] = w[side] << 8u;      // an I2S slot: left-justified (audio_i2s_multi.c:217-226)
                            }
                        }
                        // (words that are zero whatever the samples — the sub while it is off, a pair whose outputs are both disabled but
                        //  whose delay lines still run — are not stored under DSPI_OUT_ENABLED_ONLY)
                        const bool silent = is_sub ? !(sub_active && oc[N - 1].enabled) : word_scale[is_sub ? 0 : pr_] == 0.0f;
                        if (!fl || (a.skip_silent && silent)) continue;
                        if (is_sub) {
                            if (a.sub) {
                                if (a.tiled_out) sk_st2(reinterpret_cast<uint32_t *>(a.sub) + ((size_t)wg * F + frame0 + j) * ROWP + ocol, w[0], one, two);
                                else {
                                    if (one) a.sub[(size_t)stream * F + frame0 + j] = (int32_t)w[0].x;
                                    if (two) a.sub[(size_t)(stream + 1) * F + frame0 + j] = (int32_t)w[0].y;
                                }
                            }
                        } else if (a.pairs) {
                            if (a.tiled_out) {
                                uint32_t *dst = reinterpret_cast<uint32_t *>(a.pairs) + (((size_t)wg * (N - 1) + 2 * pr_) * F + frame0 + j) * ROWP + ocol;
                                sk_st2(dst, w[0], one, two);
                                sk_st2(dst + F * ROWP, w[1], one, two);
                            } else if (SPDIF) {      // DSPI_OUT_SPDIF (its own instance of the kernel: the encoder in every instance cost the plain ones registers): the frame's two subframes (sample_encoding.h:27-47), sixteen bytes per frame and stream
                                const uint32_t pos = (a.spdif_pos + (uint32_t)((frame0 + j) % 192u)) % 192u;
                                if (one) *reinterpret_cast<spdif_u4 *>(a.pairs + (((size_t)(stream - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 4) = spdif_frame(w[0].x, w[1].x, pos, sp_lo, kSpdifStatusHi);
                                if (two) *reinterpret_cast<spdif_u4 *>(a.pairs + (((size_t)(stream + 1 - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 4) = spdif_frame(w[0].y, w[1].y, pos, sp_lo, kSpdifStatusHi);
                            } else {      // the firmware's pair buffer: L, R interleaved — eight bytes per frame, a wave writes whole lines
                                if (one) *reinterpret_cast<v2u *>(a.pairs + (((size_t)(stream - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 2) = v2u{w[0].x, w[1].x};
                                if (two) *reinterpret_cast<v2u *>(a.pairs + (((size_t)(stream + 1 - a.pairs_stream0) * P + pr_) * F + frame0 + j) * 2) = v2u{w[0].y, w[1].y};
                            }
                        }
                    }
                    // the packet's output peaks: maximum over the wave's frames, then the words of usb_audio.c:915-923 / :945-951
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        if (is_sub && side) break;
                        const int o = side ? o1_ : o0_;
                        if (!oc[o].metered) continue;
                        const v2f m = v2f{sk_wave_max(opk[side].x), sk_wave_max(opk[side].y)};
                        v2u p16;
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            p16[c] = (uint32_t)(fminf(1.0f, m[c]) * 32767.0f);
                            if (m[c] > 1.001f) s.clip[c] |= 1u << (2 + o);
                        }
                        if (lane == (uint32_t)(2 + o)) pkw = p16;
                    }
                }
                if (lane < (uint32_t)sm.n_ch && ch_mine) {
                    if (a.peaks) {
                        if (one) a.peaks[((size_t)stream * n_blocks + k) * sm.n_ch + lane] = (uint16_t)pkw.x;
                        if (two) a.peaks[((size_t)(stream + 1) * n_blocks + k) * sm.n_ch + lane] = (uint16_t)pkw.y;
                    }
                    if (k == (int)n_blocks - 1) sk_st2(gs + (size_t)(sm.peaks + lane) * ROWP, pkw, one, two);      // the last packet's meters stay in the state
                }
                if (flags & IF_ANY_DELAY) s.widx = (s.widx + B) & ((uint32_t)sm.max_delay - 1u);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int h = 0; h < kPer; ++h) {
            if (!ow_live[h]) continue;
            const uint32_t opi = (split ? lp : (uint32_t)ow + (uint32_t)C::emit_waves * h);
            const bool one = sk_ha(hm, opi), two = sk_hb(hm, opi);
            uint32_t *gs = gs0 + (part * kSkPairs + opi) * 2u;
            if (!split || ow == 0) {
                sk_st2(gs + (size_t)sm.widx * ROWP, os[h].widx, one, two);
                sk_st2(gs + (size_t)(sm.mute + 0) * ROWP, os[h].loading, one, two);
                sk_st2(gs + (size_t)(sm.mute + 1) * ROWP, os[h].counter, one, two);
                sk_st2(gs + (size_t)(sm.mute + 2) * ROWP, as_v2u(os[h].smooth), one, two);
                // the leveller is off and its rings are not touched here, but the ring position moves on by the launch's frames as in
                // every other chain kernel: a stream without the leveller stays on the position of its row's streams that run it
                sk_st2(gs + (size_t)sm.ring_pos * ROWP, (os[h].rpos + (uint32_t)F) & (uint32_t)(kRingLen - 1), one, two);
            }
            if (one) atomicOr(gs + (size_t)(sm.clip + 0) * ROWP, os[h].clip.x);      // sticky bits: OR-ed into the stream's word (fetch_status ORs the slots)
            if (two) atomicOr(gs + (size_t)(sm.clip + 0) * ROWP + 1, os[h].clip.y);
        }
    }
}

// ---- the output rows (EQO): row = pair x output, waves C::mwaves .. C::mwaves + C::owaves - 1, one batch behind the master rows ----
// stage 0: the matrix mix of the post-crossfeed samples (usb_audio.c:753-779, the statements of output_item_pk), stages 1-10: the output's
// EQ bands when it runs (enabled, not muted, not bypassed: usb_audio.c:877-890), stage 11: the sample goes to LDS for the output waves.
template <bool FMA, bool PP>
__device__ __forceinline__ void sk_out_rows(const KArgs &a, SkShared<true> &sh, ImgPtr img, const DevImage *im, uint32_t wg, uint32_t part, uint32_t pmask, uint32_t hm, int ow, uint32_t lane) {
    typedef SkCfg<true> C;
    constexpr StateMap sm = make_state_map(1);
    constexpr uint32_t N = (uint32_t)sm.n_out;
    const uint32_t flags = img->flags;
    const uint32_t B = a.block_len, n_blocks = a.n_blocks, total = n_blocks * B;
    uint32_t *gs0 = a.state + (size_t)wg * sm.n_slots * ROWP;
    const uint32_t r = (uint32_t)ow * 4u + (lane >> 4), l = lane & 15u;
    const bool row_ok = r < (uint32_t)C::orows;
    const uint32_t pi = row_ok ? r / N : 0u, o = row_ok ? r % N : 0u;
    const bool row_live = row_ok && ((pmask >> pi) & 1u);
    const uint32_t col = (part * (uint32_t)C::pairs + pi) * 2u;
    const bool is_sub = o == N - 1u, processed = !is_sub || (flags & IF_SUB_ACTIVE);
    const bool enabled = (img->out_enabled >> o) & 1u, muted = (img->out_mute >> o) & 1u, bypassed = (img->ch_bypassed >> (2u + o)) & 1u;
    const bool eq_on = row_ok && processed && enabled && !muted && !bypassed;
    typedef typename SkNum<PP>::type NT;
    const SkPairImg pim = sk_pair_img<PP>(a, im, wg, col, row_live && sk_ha(hm, pi), row_live && sk_hb(hm, pi));
    const bool gl_nz = im->mix[0][o].f != 0.0f, gr_nz = im->mix[1][o].f != 0.0f;      // (per-lane loads: the output differs from row to row; the zero pattern is the structure's)
    const NT gl = sk_num<PP>(pim, [o](const DevImage *q) { return q->mix[0][o].f; }), gr = sk_num<PP>(pim, [o](const DevImage *q) { return q->mix[1][o].f; });
    const bool first_l = FMA ? !gr_nz : gl_nz, both = enabled && gl_nz && gr_nz, zero = !enabled || (!gl_nz && !gr_nz);
    const NT g1 = first_l ? gl : gr;
    uint32_t kind = K_BYPASS;
    NT c0 = NT(0.0f), c1 = NT(0.0f), c2 = NT(0.0f), c3 = NT(0.0f), c4 = NT(0.0f), c5 = NT(0.0f);
    v2f s1 = splat(0.0f), s2 = splat(0.0f);
    int slot1 = -1, slot2 = -1;
    if (l >= 1u && l <= (uint32_t)kBands && eq_on) {
        const DevBand *bd = &im->eq[2u + o][l - 1u];
        kind = bd->kind; sk_band_nums<PP>(pim, im, bd, c0, c1, c2, c3, c4, c5);
        slot1 = sm.eq + (int)(((2u + o) * kBands + (l - 1u)) * 2u); slot2 = slot1 + 1;
        if (row_live) {
            s1 = as_v2f(*reinterpret_cast<const v2u *>(gs0 + (size_t)slot1 * ROWP + col));
            s2 = as_v2f(*reinterpret_cast<const v2u *>(gs0 + (size_t)slot2 * ROWP + col));
        }
    }
    const bool is_bq = kind == K_BIQUAD, is_lp = kind == K_SVF_LP, is_hp = kind == K_SVF_HP, is_pk = kind == K_SVF_PK, is_sh = kind == K_SVF_SHELF;
    const bool is11 = l == (uint32_t)kSkOutDepth && row_ok;
    const bool any_bq = __any(is_bq), any_oth = __any(is_lp || is_hp || is_sh), any_pk = __any(is_pk);      // wave-uniform
    v2f sq1 = s1, sq2 = s2;
    v2f o0 = splat(0.0f);
    const uint32_t G = min((uint32_t)kSkMaxG, B >= (uint32_t)kSkMaxB ? 1u : (uint32_t)kSkMaxB / B);
    const uint32_t mrowL = 2u * pi, mrowR = 2u * pi + 1u;
    auto mix = [&](v2f xl, v2f xr) {
        const v2f t1 = (first_l ? xl : xr) * g1;
        const v2f t2 = FMA ? mad2<true>(gl, xl, t1) : t1 + xr * gr;
        v2f m = both ? t2 : t1;
        return zero ? splat(0.0f) : m;
    };
    __syncthreads();                   // iteration 0: the master rows' fill
    uint32_t it = 1;
    const bool wave_live = __any(row_live);      // (see sk_systolic)
    for (int p0 = -1; p0 < (int)n_blocks; p0 = p0 < 0 ? 0 : p0 + (int)G, ++it) {
        if (!wave_live) { __syncthreads(); continue; }
        // the master rows' previous iteration: buffer (it - 1) & 1; their fill left this group's fill (kSkOutDepth frames) behind its
        // own kSkDepth steps, a batch starts at index 0
        const v2f (*xi)[kSkMaxB + 1] = sh.xout[(it - 1u) & 1u];
        v2f (*yo)[kSkMaxB] = sh.yout[it & 1u];
        const uint32_t off = p0 < 0 ? (uint32_t)kSkDepth : 0u;
        const uint32_t len = p0 < 0 ? (uint32_t)kSkOutDepth : (min((uint32_t)p0 + G, n_blocks) - (uint32_t)p0) * B;
        const uint32_t f0 = p0 < 0 ? 0u : (uint32_t)p0 * B + (uint32_t)kSkOutDepth;      // the frame stage 0 takes in step 0
        v2f nl = xi[mrowL][off], nr = xi[mrowR][off];
        // Steady steps: every stage has a frame, i.e. stage 0's frame lies inside the launch — all of a batch but the launch's last one, of
        // which the first total - f0 steps are (a launch of ONE packet, the firmware's own rhythm, used to run entirely on the guarded loop).
        const uint32_t len_s = p0 >= 0 && f0 < total ? min(len, total - f0) : 0u;
        if (len_s) {
            // (round 6: hand-tuned as sk_systolic's step — stage 11's store under EXEC := its four lanes in assembly, one DPP block, two steps per iteration)
            const uint32_t y_addr = (uint32_t)(uintptr_t)&yo[r][0];
            const unsigned long long m11 = __ballot(is11);
            auto run = [&](auto bq_, auto pk_, auto oth_) {
                constexpr bool BQ = decltype(bq_)::value != 0, PKF = decltype(pk_)::value != 0, OTH = decltype(oth_)::value != 0;
                auto step = [&](uint32_t j, v2f x) {                  // x: the mix of this frame (stage 0's input)
                    sk_shr1_into(x, o0);
                    v2f out = x;
                    if (PKF || OTH) {
                        const v2f v3 = x - s2;
                        const v2f v1 = mad2<FMA>(c0, s1, c1 * v3);
                        const v2f v2 = mad2<FMA>(c2, v3, mad2<FMA>(c1, s1, s2));
                        s1 = mad2<FMA>(2.0f, v1, -s1);
                        s2 = mad2<FMA>(2.0f, v2, -s2);
                        const v2f A = mad2<FMA>(c3, v1, x);
                        if (PKF) out = is_pk ? A : out;
                        if (OTH) {
                            out = is_lp ? v2 : out;
                            out = is_hp ? A - v2 : out;
                            out = is_sh ? mad2<FMA>(c5, v2, mad2<FMA>(c3, x, c4 * v1)) : out;
                        }
                    }
                    if (BQ) {
                        const v2f y = mad2<FMA>(c0, x, sq1);
                        sq1 = mad2<FMA>(c1, x, -(c3 * y)) + sq2;
                        sq2 = mad2<FMA>(c2, x, -(c4 * y));
                        out = is_bq ? y : out;
                    }
                    o0 = out;
                    sk_lds_store_masked(y_addr + j * (uint32_t)sizeof(v2f), x, m11);      // stage 11 hands its input on
                };
                uint32_t j = 0;
                for (; j + 2u <= len_s; j += 2u) {
                    const v2f ma = mix(nl, nr);
                    const v2f l1 = xi[mrowL][j + 1], r1 = xi[mrowR][j + 1];      // (the rows have a spare element)
                    step(j, ma);
                    const v2f mb = mix(l1, r1);
                    nl = xi[mrowL][j + 2]; nr = xi[mrowR][j + 2];
                    step(j + 1u, mb);
                }
                if (j < len_s) { const v2f ma = mix(nl, nr); nl = xi[mrowL][j + 1]; nr = xi[mrowR][j + 1]; step(j, ma); }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the assembly's stores are not in the compiler's count)
            };
            auto run_o = [&](auto bq_, auto pk_) { if (any_oth) run(bq_, pk_, SkC<1>{}); else run(bq_, pk_, SkC<0>{}); };
            auto run_p = [&](auto bq_) { if (any_pk) run_o(bq_, SkC<1>{}); else run_o(bq_, SkC<0>{}); };
            if (any_bq) run_p(SkC<1>{}); else run_p(SkC<0>{});
        }
        {   // the fill, and the drain at the launch's end: a stage may have no frame in a step
#pragma unroll 1
            for (uint32_t j = len_s; j < len; ++j) {
                const v2f m = mix(nl, nr);
                nl = xi[mrowL][off + j + 1]; nr = xi[mrowR][off + j + 1];
                const v2f x = sk_shr1(o0, m);
                const uint32_t fj = f0 + j;                              // stage l works on frame fj - l
                const bool act = fj >= l && fj - l < total;
                if (act) {
                    if (l == 0u) o0 = x;
                    else if (l <= (uint32_t)kBands) o0 = is_bq ? sk_band<FMA>(kind, x, sq1, sq2, c0, c1, c2, c3, c4, c5) : sk_band<FMA>(kind, x, s1, s2, c0, c1, c2, c3, c4, c5);
                    else if (is11) yo[r][fj - l - (uint32_t)(p0 < 0 ? 0 : p0) * B] = x;      // (never in the fill: fj < l there)
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();                   // the output waves' last batch
    if (row_live && slot1 >= 0 && kind != K_BYPASS) {      // (a bypassed band's state is left alone, see sk_systolic)
        sk_st2(gs0 + (size_t)slot1 * ROWP + col, as_v2u(is_bq ? sq1 : s1), sk_ha(hm, pi), sk_hb(hm, pi));
        sk_st2(gs0 + (size_t)slot2 * ROWP + col, as_v2u(is_bq ? sq2 : s2), sk_ha(hm, pi), sk_hb(hm, pi));
    }
}

template <bool FMA, bool PCM24, bool EQO = false, bool SPDIF = false, bool PP = false>
__global__ __launch_bounds__(64 * kSkWaves) void chain_kernel_skew(KArgs a) {      // (output rows: 140 VGPRs, one workgroup per CU; capped at 128 for two: 2 % slower up to 1 024 streams, 10 % faster at 2 048)
    typedef SkCfg<EQO> C;
    extern __shared__ __attribute__((aligned(16))) uint32_t sk_lds[];
    SkShared<EQO> &sh = *reinterpret_cast<SkShared<EQO> *>(sk_lds);
    // one work item per workgroup (the host cuts a row's item into its non-empty parts): image in the low bits, part above (kSkPartShift)
    const WgItem item = a.items[blockIdx.x];
    const uint32_t part = item.image >> kSkPartShift, image = item.image & ((1u << kSkPartShift) - 1u);
    const uint32_t pa = (uint32_t)(item.mask >> (part * C::pairs)) & ((1u << C::pairs) - 1u);       // first streams of the workgroup's pairs in this launch
    const uint32_t pb = (uint32_t)(item.mask1 >> (part * C::pairs)) & ((1u << C::pairs) - 1u);      // second streams
    const uint32_t pmask = pa | pb, hm = pa | (pb << 16);
    if (pmask == 0u) return;
    ImgPtr img = to_const(a.img + image);
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // all groups pass the same barriers: one after the fill, one per batch, one (with output rows: two) at the end
    if (wave < C::mwaves) sk_systolic<FMA, PCM24, EQO, PP>(a, sh, img, a.img + image, item.wg, part, pmask, hm, wave, lane);
    else if (EQO && wave < C::mwaves + C::owaves) {
        if constexpr (EQO) sk_out_rows<FMA, PP>(a, sh, img, a.img + image, item.wg, part, pmask, hm, wave - C::mwaves, lane);
    } else {
        sk_outputs<FMA, EQO, SPDIF, PP>(a, sh, img, a.img + image, item.wg, part, pmask, hm, wave - C::mwaves - C::owaves, lane);
        __syncthreads();
    }
}
