// dmel_fwd_body.inc -- the fused forward kernel, included twice by dmel_fwd.hip: DMEL_FWD_MULTI = 0 makes dmel_fwd_kernel (the scalar layer), 1
// makes dmel_fwd_multi_kernel (the multi-window layer, FwdParams::ch_out > 0).  dmel_fwd_len.hip includes it a third time with DMEL_FWD_LEN = 1:
// dmel_fwd_len_kernel, the scalar layer over clips of per-clip lengths (FwdLenParams).  The FWD_* names below expand, for the scalar kernel, to
// exactly the tokens it was written with, so that its code does not change.
// dmel_fwd_band.hip includes it with DMEL_FWD_MULTI = 1 and DMEL_FWD_BAND = 1: dmel_fwd_band_kernel (BandSplitMelSpectrogram, FwdBandParams) -- the
// multi-window kernel's channel addressing, but all channels write ONE (B, 1, M, T) image and channel c only its rows [e_c, e_c+1): the
// contraction work of the other rows is skipped where a whole tile / phase lies outside them and every store site is confined to them.
// dmel_fwd_fb_len.hip includes it with DMEL_FWD_LEN = 1 and DMEL_FWD_FB = 1: dmel_fwd_fb_len_kernel (FwdFbLenParams), the length-aware builds a trained
// filterbank needs -- kTrainH, kSpec and a kTrain whose saved spectrogram follows the lengths; what differs sits behind DMEL_FWD_FB.
// The two axes compose: DMEL_FWD_LEN = 1 on top of DMEL_FWD_MULTI (and DMEL_FWD_BAND) makes dmel_fwd_multi_len_kernel (dmel_fwd_multi_len.hip,
// FwdMultiLenParams) and dmel_fwd_band_len_kernel (dmel_fwd_band_len.hip, FwdBandLenParams): the K-window layers over clips of per-clip lengths.
#if DMEL_FWD_MULTI
#define FWD_BO bo
#define FWD_LAM lam_args
#define FWD_WIN2 win2
#define FWD_LEADER grid_leader
#if DMEL_FWD_BAND && DMEL_FWD_LEN
#define FWD_KERNEL dmel_fwd_band_len_kernel
#define FWD_PARAMS FwdBandLenParams
#elif DMEL_FWD_BAND
#define FWD_KERNEL dmel_fwd_band_kernel
#define FWD_PARAMS FwdBandParams
#elif DMEL_FWD_LEN
#define FWD_KERNEL dmel_fwd_multi_len_kernel
#define FWD_PARAMS FwdMultiLenParams
#else
#define FWD_KERNEL dmel_fwd_multi_kernel
#define FWD_PARAMS FwdParams
#endif
#else
#define FWD_BO b
#define FWD_LAM p.lam
#define FWD_WIN2 p.win2
#define FWD_LEADER blockIdx.x == 0
#if DMEL_FWD_LEN && DMEL_FWD_FB
#define FWD_KERNEL dmel_fwd_fb_len_kernel
#define FWD_PARAMS FwdFbLenParams
#elif DMEL_FWD_LEN
#define FWD_KERNEL dmel_fwd_len_kernel
#define FWD_PARAMS FwdLenParams
#else
#define FWD_KERNEL dmel_fwd_kernel
#define FWD_PARAMS FwdParams
#endif
#endif
// sample-space bounds of a clip: p.L (also the row stride of x) and fl32(1 / L), or the clip's own length Lc (dmel_fwd_len_kernel); its
// frames: p.T, or Tc
// FWD_PAD_MEL(t, v): the mel power v of frame t, or 0 in a pad frame -- the pair modes' epilogue: there a pad frame shares its complex FFT
// with a frame of the clip and would carry that frame's rounding noise
#if DMEL_FWD_LEN
#define FWD_LC Lc
#define FWD_INV_L inv_Lc
#define FWD_TC Tc
#define FWD_PAD_MEL(t, v) ((t) < Tc ? (v) : 0.f)
#else
#define FWD_LC p.L
#define FWD_INV_L p.inv_L
#define FWD_TC p.T
#define FWD_PAD_MEL(t, v) v
#endif
#ifndef DMEL_TWC
#define DMEL_TWC 8
#endif
// dmel_fwd_band_kernel: 1 = tiles / phases that hold none of the channel's rows are not contracted; 0 = every row is contracted and the stores
// alone are masked (diagnostic builds: the comparison of NOTEBOOK R8.1)
#ifndef DMEL_BAND_SKIP
#define DMEL_BAND_SKIP 1
#endif
template <int N, int MODE, int TPW>
__global__ void __launch_bounds__((geom_mode<N, MODE>().THREADS), (geom_mode<N, MODE>().MINW)) FWD_KERNEL(FWD_PARAMS p)
{
    constexpr FftGeom g = geom_mode<N, MODE>();
    constexpr int R = g.R, C = g.C, G = g.G, FPW = g.FPW, PASSES = g.PASSES, SLOTS = g.SLOTS, MT = g.MT;
    constexpr int WAVES = g.WAVES, NLOC = g.NLOC, THREADS = g.THREADS;
    constexpr int LB = ilog2(R);
    constexpr int EXS = g.EX_STRIDE, SS = g.SLOT_STRIDE_F2;
    constexpr bool PAIR = (MODE == kInfer || MODE == kSpec);    // two frames share one complex FFT
    constexpr bool IS_SPEC = (MODE == kSpec || MODE == kSpecTrain);
    constexpr bool HSPLIT = (MODE == kTrainH);                  // dense contraction on the bf16 matrix pipe: PD kept as four bf16 planes
#ifndef DMEL_DIT_MASK
#define DMEL_DIT_MASK (~0)
#endif
    // register radix core: decimation in time with Linzer-Feig butterflies (194 packed operations per 32 points) or the round-4
    // decimation in frequency (228); bit log2(N) of DMEL_DIT_MASK selects (diagnostic builds)
    // (measured, training: n_fft 4096 145.2 -> 138.5 us at the reference's ESC-50 shape, n_fft 1024 -1 % in many-round launches; n_fft 2048
    // with the round-4 contraction 48.0 -> 49.0 us at config 3, 70.2 -> 72.4 at config 5 -- eight spilled registers -- but 46.9 -> 46.0 and
    // 71.9 -> 70.3 with the wave-local contraction: there it stays)
    constexpr bool WLC = mode_wlc(MODE);                        // wave-local contraction: see phase 2
    constexpr bool USE_DIT = ((DMEL_DIT_MASK >> ilog2(N)) & 1) != 0 && (N != 2048 || WLC);
    constexpr bool TRAINLIKE = (MODE == kTrain || MODE == kTrainH || WLC);
    constexpr int NHS = hsplit_plane_stride(N);                 // bf16 entries per plane (bins 0 .. N/2 + padding to 16 bytes)
    static_assert(!HSPLIT || (N >= kHsplitMinNfft && N <= kHsplitMaxNfft), "kTrainH: frames inside one wave, N/2 a multiple of 32");
    constexpr int FPT = PAIR ? 2 * SLOTS : SLOTS;               // frames per tile
    constexpr int F = N / 2 + 1;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    v2f* lds = reinterpret_cast<v2f*>(smem_raw);
    float2* wtab = reinterpret_cast<float2*>(smem_raw + g.AUX_OFF);   // window table (phase 1 only)
    float* red = reinterpret_cast<float*>(smem_raw + g.RED_OFF);
    constexpr bool WIN_LDS = g.WIN_LDS != 0;
    // radix-C twiddles through LDS: the table has R*C entries but a wave-wide global load of it still moves 512 B
    constexpr bool TW2_LDS = (C > 1) && (N <= 2048);
    float2* tw2l = reinterpret_cast<float2*>(smem_raw + g.RED_OFF + kRedBytes);
    // the half-tile exchange of phase 2 (8 waves) lives where the window table does: a second tile needs the table back
    constexpr bool WIN_ALIASED = WIN_LDS;
    // compact layouts (dmel_kernels.h): pairing pass through ds_bpermute, transposition one plane at a time, half window table
    constexpr bool BPERM = g.PAIRING == kPairBperm, PLANE = g.PAIRING == kPairPlane, SPLIT = g.SPLIT != 0, WIN_SYM = g.WIN_SYM != 0;
    constexpr bool KEEPZ = BPERM || PLANE;                      // the spectrum stays in registers until the pairing pass
    constexpr int WPF = g.WPF;                                  // waves per frame (n_fft 8192: 2, 16384: 4)
    static_assert(!BPERM || (G <= 64 && PASSES == 1 && (G == 64 || C == 1 || (WLC && C == 2))), "the bpermute pairing pass: whole frames inside one wave");
    static_assert(!SPLIT || KEEPZ, "a one-plane slot cannot hold the whole spectrum");
    static_assert(!WIN_SYM || G <= 64, "half window table: frames inside one wave");
    static_assert(WPF == 1 || (PLANE && SPLIT && PASSES == 1 && !WIN_LDS), "frames spread over several waves exchange through planes");
    static_assert(!PLANE || G >= 64, "plane pairing: whole waves per frame");
    static_assert(!WLC || (BPERM && WPF == 1 && PASSES == 1 && TPW == 1 && wlc_size(N) && FPW <= 2), "kTrainW: whole frames inside one wave, at most four (frame, P | D) rows per wave");
    constexpr int WPT = (N / 2 + THREADS - 1) / THREADS;       // window entries a thread computes (and keeps when TPW > 1)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 shares an L2).  Re-labelling them so
    // that each XCD gets a CONTIGUOUS range of tiles puts the tiles of one clip on one L2: their
    // overlapping sample reads hit, and the 32-byte output pieces that together make up whole lines
    // of out/tangent merge there before going to HBM.  Speed only; any placement is correct.
    int wg = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, rr = nwg & 7, xcd = wg & 7;
        // (the two workgroups that share a CU -- local indices i and i + 32 of an XCD's 64 at config 2 -- given the two halves of ONE
        // clip, so that the second pass over the clip hits L1: 19.99 against 20.05 us, not kept)
        wg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (wg >> 3);
    }
    // multi-window layer: the channel slot comes out of the relabelled index, so that a channel's tiles keep the placement above;
    // its lambd words, window table and output rows are the channel's (dmel_kernels.h: lam_for_channel).  bo = the output's clip row.
#if DMEL_FWD_MULTI
    const int slot = wg / p.ch_grid;
    wg -= slot * p.ch_grid;
    const int ch = (int)((p.ch_list >> (4 * slot)) & 15u);
    const bool grid_leader = wg == 0;
    const LamArgs lam_args = lam_for_channel(p.lam, ch, slot, p.ch_roles, p.ch_val);
    const float2* const win2 = p.win2 + (size_t)ch * kMaxNfft;
#endif
    const int b = wg / p.wgs_per_clip;
#if DMEL_FWD_MULTI
#if DMEL_FWD_BAND
    // one image for all channels; this channel's rows [e_lo, e_hi): two scalar loads from the kernel arguments, uniform over the workgroup
    const int bo = b;
    const int e_lo = __builtin_amdgcn_readfirstlane(p.band_edges[ch]), e_hi = __builtin_amdgcn_readfirstlane(p.band_edges[ch + 1]);
#else
    const int bo = b * p.ch_out + ch;
#endif
#endif
#if DMEL_FWD_LEN
    // the clip is x[b, :Lc] (one scalar load: uniform over the workgroup) with Tc = Lc / hop + 1 frames; the frames past them are pad frames.
    // A length outside 1 ... L makes the clip's rows NaN (behind the coverage check below); until then it reads as 1, so that every load of the
    // workgroup stays inside the row
    const int len_raw = *(const __attribute__((address_space(4))) int*)(p.lengths + b);
    const bool len_ok = len_raw >= 1 && len_raw <= p.L;
    const int Lc = __builtin_amdgcn_readfirstlane(len_ok ? len_raw : 1);
    const int Tc = Lc / p.hop + 1;
    const float inv_Lc = 1.0f / (float)Lc;
#endif
    const int tile0 = (wg % p.wgs_per_clip) * TPW;              // first tile of this workgroup inside its clip
    STAMP(0);
    STAMP_PLACE();
#ifdef DMEL_ABLATE
    // timing ablations (tools/ablate.py builds its own library with -DDMEL_ABLATE; never in libdmel_hip.so)
    const bool dbg_skip_fft = (p.flags & 0x200u) != 0;
    const bool dbg_skip_gemm = (p.flags & 0x100u) != 0;
#else
    constexpr bool dbg_skip_fft = false;
#endif

#ifdef DMEL_ABLATE
    // timing experiment: the workgroups of the first round whose CU-local slot is odd start late by (flags >> 24) x 1024 cycles, so that
    // the two workgroups a CU holds stay out of step for the rest of a many-round launch
    if ((p.flags & 0x400000u) && blockIdx.x < 512u) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        if ((hw >> 16) & 1u) for (unsigned i = 0; i < (p.flags >> 24) * 16u; ++i) __builtin_amdgcn_s_sleep(1);
    }
#endif
    // the batch: by address, or (DMEL_FLAG_X_INDIRECT) through a pointer cell read with a scalar load -- a captured step is handed a
    // new batch by rewriting 8 bytes
    const float* xbase = p.x;
    if (p.x_ind) { typedef const float* cfp; xbase = *(const __attribute__((address_space(4))) cfp*)p.x_ind; }
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(xbase + (size_t)b * p.L, (unsigned)FWD_LC * 4u);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.ent_b, (unsigned)p.ent_b_floats * 4u);

    // ---- what phase 2 needs from global memory: (ks0, nks, boff, tile) of this wave's mel runs in group 0 and their
    // first NBPRE B fragments (all of them for the HTK bank at the usual sizes).  Requested after the FFT of a tile, when
    // its registers are free: the pairing pass and the barrier behind it cover the round trip, nothing in phase 2 waits.
    constexpr int NBPRE = g.NBPRE;
    int4 tr0[NLOC];
    float bpre[NLOC][NBPRE];
    auto fetch_bpre = [&]() {
        if constexpr (!IS_SPEC && !WLC) {
            static_for<0, NLOC>([&](auto l) {
                constexpr int loc = decltype(l)::value;
                tr0[loc] = p.tile_ranges[wave * NLOC + loc];
            });
            // one 64-bit base per lane, compile-time offsets from it
            const float* pre_lane = p.ent_pre + ((unsigned)(wave * (NLOC * NBPRE * 64)) + (unsigned)lane);
            static_for<0, NLOC>([&](auto l) {
                constexpr int loc = decltype(l)::value;
                // fixed layout (wave, run, k-step, lane): the address does not wait for tile_ranges; the number of real groups of
                // 4 k-steps comes with the kernel arguments (scalar load), so the padding of short runs is not fetched
                const int ng = p.pre_groups[wave * NLOC + loc];
                static_for<0, NBPRE / 4>([&](auto qq) {
                    constexpr int q4 = decltype(qq)::value;
                    if (q4 < ng) {
                        static_for<0, 4>([&](auto u) {
                            constexpr int u4 = q4 * 4 + decltype(u)::value;
                            bpre[loc][u4] = pre_lane[(loc * NBPRE + u4) * 64];
                        });
                    } else {
                        // defined on every path: the registers are then dead between two tiles instead of carrying the
                        // previous tile's values through the next FFT
                        static_for<0, 4>([&](auto u) { bpre[loc][q4 * 4 + decltype(u)::value] = 0.f; });
                    }
                });
            });
        }
    };

    // kTrainW: what its phase 2 needs from global memory -- the lane table of the first two phases and the first groups of B operands
    // of phase 0 -- is requested where fetch_bpre() is (behind the second radix stage: the pairing pass covers the round trips); the
    // ring is refilled for the next phase in front of each phase's epilogue.  (Asked for where they are used, each phase began
    // with two dependent round trips: 5 400 cycles per wave for 88 MFMAs and two epilogues, tools/stamps.py.)
#ifndef DMEL_WL_DEPTH
#define DMEL_WL_DEPTH 6
#endif
#ifndef DMEL_WL_EARLY
#define DMEL_WL_EARLY 0
#endif
#ifndef DMEL_WL_NEXT
#define DMEL_WL_NEXT 1
#endif
    constexpr int WL_DEPTH = DMEL_WL_DEPTH;                     // groups of four steps (16 bytes per lane) in the ring
    constexpr int WL_EARLY = DMEL_WL_EARLY;                     // 1: lane tables requested before the pairing pass, 2: the ring of phase 0 too
    floatx4 wl_ring[WLC ? WL_DEPTH : 1];
    int2 wl_li[2];
    const __amdgpu_buffer_rsrc_t rbw = make_rsrc(WLC ? (const void*)p.wl_b4 : (const void*)p.x, WLC ? (unsigned)p.wl_total4 * 1024u : 0u);
    // BUFFER loads on purpose: with plain loads InstCombine folds the ring's phi(load, load) into load(phi(address)) at the loop
    // header and every group waits a cache round trip in front of its first use; an intrinsic call is not folded.  Groups past the
    // end of a phase re-read its last group.
#ifndef DMEL_WL_UNCOND
#define DMEL_WL_UNCOND 1
#endif
    // DMEL_WL_UNCOND (round 6): EVERY ring load is issued -- a group past the end of its phase re-reads the phase's last group, which nobody
    // uses.  With conditional loads the compiler cannot know how many loads follow the one a slot waits for (a slot's `s_waitcnt vmcnt(N)`
    // is only safe if N loads were issued behind it), so every turn of the ring opened with `vmcnt(0)`: the refill requested two
    // instructions earlier was waited for in full, ~300 cycles per turn, 15-20 turns per tile at n_fft 2048 (NOTEBOOK R5.20).  Now the ring is
    // a fixed pattern of WL_DEPTH loads per turn and the waits are `vmcnt(WL_DEPTH - 1)`.
    auto wl_bload = [&](floatx4& dst, int grp, int n4, int boff4) {
#ifdef DMEL_ABLATE
        if (p.flags & 0x10000u) return;                          // timing only: no B operand loads
#endif
        if constexpr (DMEL_WL_UNCOND) {
            // the table index stays inside [0, wl_total4 - 1] whatever the phase holds: a phase of quads whose bands are all empty (many mel bands on few
            // bins) has n4 = 0, and the buffer's range check does not cover the scalar offset
            // (`n4` carries the phase's LAST table index here -- wl_last() -- so that a load costs one scalar add and one scalar min)
            const int gi = boff4 + grp < n4 ? boff4 + grp : n4;
            dst = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rbw, lane * 16, __builtin_amdgcn_readfirstlane(gi) * 1024, 0));
        } else
        if (grp < n4) dst = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rbw, lane * 16, (boff4 + __builtin_amdgcn_readfirstlane(grp)) * 1024, 0));
    };
    // last table index a phase of n4 groups at offset boff4 may read: inside [0, wl_total4 - 1] even for an empty phase
    auto wl_last = [&](int n4, int boff4) -> int {
        int l = boff4 + n4; l = l < p.wl_total4 ? l : p.wl_total4; l -= 1;
        return l > 0 ? l : 0;
    };
    auto wl_ring_init = [&](int n4, int boff4) {
        if constexpr (DMEL_WL_UNCOND) n4 = wl_last(n4, boff4);
        // (a slot whose group does not exist in this phase is never used -- the tail groups are guarded -- so it is "defined" by an empty asm
        // statement instead of four zeros: 24 moves less per ring start, 48-72 vector instructions per wave)
        if constexpr (WLC) static_for<0, WL_DEPTH>([&](auto dd) { constexpr int d = decltype(dd)::value; asm volatile("" : "=v"(wl_ring[d])); wl_bload(wl_ring[d], d, n4, boff4); });
    };
    auto wl_prefetch = [&]() {
        if constexpr (WLC && WL_EARLY >= 1) {
            wl_li[0] = p.wl_lane[lane];
            wl_li[1] = p.wl_lane[(p.wl_phases > 1 ? 64 : 0) + lane];
            if constexpr (WL_EARLY >= 2) wl_ring_init(p.wl_len4[0], 0);
        }
    };

    // lane of this thread inside its frame: part of a wave (G < 64), the wave, or one of WPF waves
    const int j = (WPF > 1) ? 0 : lane / G;
    const int lg = (WPF > 1) ? (wave % WPF) * 64 + lane : lane % G;
    const int qp = lg / C, r = lg % C;
    // exchange among the lanes of one frame: a wave-level fence, or a workgroup barrier when the frame has several waves
    // (every wave of the workgroup runs the same sequence of them)
    // Frames of several waves (n_fft 8192: two, 16384: four): their waves meet at a counter in LDS -- one word per frame, words
    // 36 .. 39 of the sums' region, zeroed in the prologue -- instead of at a workgroup barrier: each wave adds one and waits until
    // the word has reached (number of meetings so far) x WPF.  A frame's waves are resident together (one workgroup), so the wait ends;
    // the frames of a workgroup no longer wait for one another between the transposition and pairing steps (nine meetings per tile).
    unsigned* fctr = reinterpret_cast<unsigned*>(red) + 36;
    unsigned fmeet = 0;
    static_assert(WPF == 1 || (WAVES / WPF <= 4 && 36 + 4 <= kRedBytes / 4), "one counter per frame of the workgroup");
    auto sync_frame = [&]() {
        if constexpr (WPF > 1) {
            fmeet += WPF;
            unsigned* c = fctr + wave / WPF;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // this wave's LDS writes are issued (LDS executes a wave's operations in order)
            if (lane == 0) __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (;;) {
                const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((int)((unsigned)__builtin_amdgcn_readfirstlane((int)v) - fmeet) >= 0) break;
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };

    // ---- samples: one register set per tile of the workgroup; tile ti + 1 is requested while tile ti is transformed.
    // Frames that lie wholly inside the clip (all but the first/last few) use plain offsets; the others clamp every index
    // into the clip and are zeroed by a select at windowing time.  (The hardware range check of buffer loads is not relied
    // upon: it covers voffset + immediate but not soffset, and hipcc chooses that split.)
    float xa[TPW][PASSES][R];
    float xb2[TPW][PAIR ? PASSES : 1][PAIR ? R : 1];
    bool inside[TPW][PASSES];
    auto load_tile = [&](auto tt) {
        constexpr int ti = decltype(tt)::value;
        const int t0 = (tile0 + ti) * FPT;
        static_for<0, PASSES>([&](auto pp) {
            constexpr int pass = decltype(pp)::value;
            const int slot = (WPF > 1) ? wave / WPF : pass * (WAVES * FPW) + wave * FPW + j;
            const int tA = PAIR ? (t0 + 2 * slot) : (t0 + slot);
            const int f0 = tA * p.hop - N / 2;                       // first sample of frame tA
            const int f1 = PAIR ? f0 + p.hop : f0;
            inside[ti][pass] = __all((f0 >= 0) && (f1 + N <= FWD_LC));
#ifdef DMEL_ABLATE
            if (p.flags & 0x2000u) inside[ti][pass] = true;      // timing only: no edge path (edge frames come out wrong)
#endif
            const int sA = f0 + lg;
            bool plain_loads = inside[ti][pass];
#ifdef DMEL_ABLATE
            if (p.flags & 0x4000u) plain_loads = true;           // timing only: unclamped loads, selects kept
#endif
            if (plain_loads) {
                static_for<0, R>([&](auto aa) {
                    constexpr int a = decltype(aa)::value;
                    xa[ti][pass][a] = buf_f32(rx, (sA + G * a) * 4);
                    if constexpr (PAIR) xb2[ti][pass][a] = buf_f32(rx, (sA + p.hop + G * a) * 4);
                });
            } else {
                static_for<0, R>([&](auto aa) {
                    constexpr int a = decltype(aa)::value;
                    xa[ti][pass][a] = buf_f32(rx, clampi(sA + G * a, FWD_LC - 1) * 4);
                    if constexpr (PAIR) xb2[ti][pass][a] = buf_f32(rx, clampi(sA + p.hop + G * a, FWD_LC - 1) * 4);
                });
            }
        });
    };

#if DMEL_FWD_LEN
    // rows of frames [t_first, t_end) of this clip without a transform: pad frames (zero mel power -- 0, or the epilogue's own log(0 + eps) --
    // and a zero tangent) or, for an invalid length, NaN.  The rows are the channel's: all M of its own image (FWD_BO), or, in the band build,
    // rows [e_lo, e_hi) of the shared one -- another group's rows are never written here
#if DMEL_FWD_BAND
#define FWD_FILL_ROWS (e_hi - e_lo)
#define FWD_FILL_ROW(i) (e_lo + (i))
#else
#define FWD_FILL_ROWS p.M
#define FWD_FILL_ROW(i) i
#endif
    auto fill_rows = [&](int t_first, int t_end, bool pad) {
        const bool do_log = (p.flags & 1u) != 0;
        const bool out_bf16 = (p.flags & 4u) != 0;
        float v = __builtin_nanf(""), tv = v;
        if (pad) {
            const float me = 0.f + p.eps;
            v = do_log ? (WLC ? fast_log(me, p.eps) : logf(me)) : 0.f;
            tv = 0.f;
        }
        if (t_end > p.T) t_end = p.T;
        const int nf = t_end - t_first;
        if (nf <= 0) return;
        for (int idx = tid; idx < FWD_FILL_ROWS * nf; idx += THREADS) {
            const int m = FWD_FILL_ROW(idx / nf), t = t_first + idx % nf;
            const size_t o = ((size_t)FWD_BO * p.M + m) * p.T + t;
            if (out_bf16) reinterpret_cast<unsigned short*>(p.out)[o] = bf16_bits(v); else p.out[o] = v;
            if (p.tangent) p.tangent[o] = tv;
        }
    };
#endif
    // ================= prologue, once per workgroup ============================================
    constexpr bool TW1_LDS = g.TW1_OFF != 0;                    // first-stage twiddles from a table in LDS (kTrainW where it fits)
    constexpr bool TW1_POW = (R >= 16) && !TW1_LDS;             // first-stage twiddles by powers: see phase 1
    float mean = 0.f;
    float2 wkeep[WPT];                                          // this thread's window entries (TPW > 1: written back per tile)
    float2 wmid = make_float2(1.f, 0.f);                        // ... and the centre entry
    const float lam_raw = lam_load(FWD_LAM);                       // a scalar load: see lam_load
    if (!dbg_skip_fft) {
        load_tile(IC<0>{});
        // The waves that hold a clip's first / last frames take the slow path (clamped loads, selects at windowing time) and every
        // other wave of their workgroup waits for them at the barrier before phase 2.  In a launch of ONE round of resident
        // workgroups (kFwdEdgeFirst, set by the host) they get instruction-issue priority over the waves they share a SIMD with:
        // 20.1 -> 19.7 us at BASELINE config 2 (training), 14.0 -> 13.7 (inference).  In launches of several rounds the same
        // priority measured 49.0 -> 52.0 us (config 3) and 73.9 -> 76.7 (config 5): there the waves of different rounds overlap
        // and a privileged wave only delays them.  (Measured and not kept, config 2: priority by wave index, one workgroup of
        // each CU first through the transforms, the contraction phase first: 20.1 against 20.1.)
        if ((p.flags & kFwdEdgeFirst) && !inside[0][0]) __builtin_amdgcn_s_setprio(2);
        // long clips: the partial sums of dmel_prep_kernel are requested here, next to the samples -- asked for where they are used
        // (behind the window table's barrier) every workgroup waited a global round trip for 64 floats
        float ps_early = 0.f;
        if (p.remove_dc && p.psum != nullptr) ps_early = (lane < p.nchunks) ? p.psum[(size_t)b * p.nchunks + lane] : 0.f;
        STAMP(1);   // loads issued
        // lambd (device scalar or by value) and the check that this launch is the n_fft the device value asks for
        // (lam_clip_scale: a clip no longer than |lambd| -- dmel_kernels.h; the table of n_fft 8192 / 16384 is dmel_prep_kernel's, scaled by the row length)
        const LamState ls0 = lam_prologue(FWD_LAM, N, FWD_LEADER && tid == 0, lam_raw);
        LamState ls1 = ls0;
        if constexpr (TRAINLIKE || MODE == kSpecTrain) { if (!p.normalize) ls1 = lam_clip_scale(ls0, g.WIN_LDS ? FWD_LC : p.L); }      // (the modes that write a tangent)
        const LamState ls = ls1;
#if DMEL_FWD_LEN && DMEL_FWD_FB
        // the trained bank's builds: a length outside 1 ... L takes the NaN loop of an uncovered launch -- the clip's rows and tangent, and its whole
        // (F, T) spectrogram (kSpec's output, or spec_out): the filterbank gradient sums such a clip over all T frames.  (A loop of its own behind
        // the coverage check cost kSpec 4 ... 6 spilled registers more than dmel_fwd_kernel's at n_fft 2048 ... 8192.)
        // A pad tile leaves through the same exit (one more return behind the coverage check cost as much).
        const bool bad_len = ls.action == kLamRun && !len_ok;
        const bool pad_tile = ls.action == kLamRun && len_ok && tile0 * FPT >= Tc;
        if (ls.action != kLamRun || bad_len || pad_tile) {
            if constexpr (!IS_SPEC) { if (pad_tile) fill_rows(tile0 * FPT, (tile0 + TPW) * FPT, true); }      // (kSpec: nothing -- the filterbank gradient stops at Tc)
            if (ls.action == kLamPoison || bad_len) {
#else
        if (ls.action != kLamRun) {
            if (ls.action == kLamPoison) {
#endif
                // no launch of this forward matched the device lambd: NaN instead of stale memory (the host raises too)
#if DMEL_FWD_BAND
                const int rows = p.M, nrows = e_hi - e_lo, row0 = e_lo;              // this channel's rows only: the other groups' stay as they are
#else
                const int rows = IS_SPEC ? F : p.M, nrows = rows;
                constexpr int row0 = 0;
#endif
                const float qn = __builtin_nanf("");
                for (int idx = tid; idx < nrows * FPT * TPW; idx += THREADS) {
                    const int rr = row0 + idx / (FPT * TPW), t = tile0 * FPT + idx % (FPT * TPW);
                    if (t >= p.T) continue;
                    const size_t o = ((size_t)FWD_BO * rows + rr) * p.T + t;
                    if (p.flags & 4u) reinterpret_cast<unsigned short*>(p.out)[o] = 0x7fc0u; else p.out[o] = qn;
                    if (p.tangent) p.tangent[o] = qn;
                }
                // ... and the saved spectrogram (B, F, T): the filterbank gradient contracts it before the next forward raises (ADVICE r04:
                // with a linear output and a finite upstream gradient, uninitialised memory reached the optimizer)
                if constexpr (TRAINLIKE) {
                    if (p.spec_out) {
                        for (int idx = tid; idx < F * FPT * TPW; idx += THREADS) {
                            const int kk = idx / (FPT * TPW), t = tile0 * FPT + idx % (FPT * TPW);
                            if (t < p.T) p.spec_out[((size_t)b * F + kk) * p.T + t] = qn;
                        }
                    }
                }
            }
            return;
        }
#if DMEL_FWD_LEN
        // a workgroup whose first frame lies past the clip transforms nothing: it writes its pad rows (or NaN rows for an invalid length) and is
        // done.  (Behind the coverage check: only the launch whose n_fft the device lambd selects writes.)
#if !DMEL_FWD_FB
        if (!len_ok || tile0 * FPT >= Tc) {
            fill_rows(tile0 * FPT, (tile0 + TPW) * FPT, len_ok);
            return;
        }
#endif
#endif
        if constexpr (WPF > 1) {
            if (tid < 4) fctr[tid] = 0u;                                  // the frames' meeting counters (sync_frame)
            __syncthreads();
        }
        // d out / d lambd = htan * (contraction of the scaled tangent spectrum): an fp64 division, done by ONE wave of the
        // workgroup and handed to the epilogue through LDS (every barrier below lies between this store and that load)
        if constexpr (TRAINLIKE || MODE == kSpecTrain) {
            if (wave == 0) { const float h = 0.5f * lam_tangent_scale(ls); if (lane == 0) red[kRedTan] = h; }
        }
        if constexpr (TW2_LDS) { if (tid < R * C) tw2l[tid] = p.tw2[tid]; }          // visible after the barrier below
        if constexpr (TW1_LDS) {
            // rows q = 1 .. R - 1 of the first-stage twiddle table, 16 bytes per thread (visible after the window table's barrier)
            constexpr int n16 = (R - 1) * G / 2;
            for (int i = tid; i < n16; i += THREADS)
                reinterpret_cast<float4*>(smem_raw + g.TW1_OFF)[i] = reinterpret_cast<const float4*>(p.tw1 + G)[i];
        }
        // Phase 2 pads every run of k-steps to a multiple of four with zero filterbank blocks and still reads the A operands of the
        // padding: bins past n_fft/2, i.e. floats 2 F .. of the slot.  In the compact layout those are the end of the transposition
        // plane -- finite data of this tile, EXCEPT the padding column of a row (row stride EXS = G + 1: one float nobody writes)
        // -- and the padding of the slot stride.  At n_fft 1024 float 1055 (bin 527, tangent row: read by the HTK bank's last mel
        // tile) and bins 528 .. 531 (a dense bank) are such holes: whatever an earlier kernel left in LDS -- a NaN pattern -- times
        // a zero coefficient poisoned the accumulator (found in round 4: a trainable-filterbank run went NaN after a few hundred
        // steps, and at once on a box whose previous process had left NaNs behind).  Everything from float 2 F to the end of the
        // slot is zeroed once per workgroup, before the barrier in front of the first transform: what the transposition writes
        // there later is finite, what it leaves out stays zero.
        if constexpr (SPLIT && !IS_SPEC) {
            constexpr int first = 2 * F, count = SS * 2 - first;                                // floats
            static_assert(count >= 0, "slot stride covers PD[0 .. N/2]");
            if constexpr (count > 0) {
                constexpr int CP = 1 << (ilog2(count - 1 > 0 ? count - 1 : 1) + 1);               // next power of two: shifts and masks, no division by `count`
                static_assert(count <= CP, "slot padding fits the zeroing loop");
#ifdef DMEL_ABLATE
                if (!(p.flags & 0x100000u))                                                      // timing only: without the zeroing
#endif
                for (int i = tid; i < SLOTS * CP; i += THREADS) {
                    const int slot = i / CP, jz = i % CP;
                    if (jz < count) reinterpret_cast<float*>(smem_raw + slot * (SS * 8))[first + jz] = 0.f;
                }
                // any thread zeroes any slot: the zeroes must land before the slot's own waves write their transposition there.  With
                // the window table in LDS the barrier behind it does that; the sizes without one (n_fft >= 8192) had NO barrier
                // before the first transform -- frames next to a clip's edge came out wrong now and then until this one went in
                // (caught by tests/test_hip_soak.py::test_no_path_depends_on_what_earlier_kernels_left_in_lds)
                if constexpr (!WIN_LDS) __syncthreads();
            }
        }
        // ---- window table into LDS (time_frequency.py:21-30): every workgroup evaluates the same fp32
        // expression, so the table is identical everywhere; this replaces a separate kernel launch
        if constexpr (WIN_LDS) {
            const float denom = ls.denom;
            float s_ww = 0.f, s_wd = 0.f;
            // w[N/2 + d] = w[N/2 - d]: entry n < N/2 is computed once and stored at n and N - n (n = 0 has no mirror);
            // the centre is exp(-0) = 1 with a zero tangent
            static_for<0, WPT>([&](auto ww_) {
                constexpr int wi = decltype(ww_)::value;
                const int n = tid + THREADS * wi;
                wkeep[wi] = make_float2(0.f, 0.f);
                if (n < N / 2) {
                    const float d = (float)n - (float)N / 2.0f;
                    const float t = d / denom;
                    float w = expf(-0.5f * (t * t));
                    if (p.win_half && n < N / 4) w = 0.f;                         // torch.stft pads a win_length = N/2 window
                    // tangent window up to a constant: w d^2 2^(-2e) (d^2 and the scaling are exact in fp32: one rounding); the
                    // factor sign 2^(2e) / (|lambd| + 1e-15)^3 is applied once per output in the epilogue (lam_tangent_scale)
                    const float dw = w * (d * d) * ls.s2;
                    wkeep[wi] = make_float2(w, dw);
                    wtab[n] = wkeep[wi];
                    // the half-length window of torch.stft sits at [N/4, 3N/4): its mirror image stops one entry short
                    const bool has_mirror = n > 0 && !(p.win_half && n <= N / 4);
                    if constexpr (!WIN_SYM) { if (n > 0) wtab[N - n] = has_mirror ? wkeep[wi] : make_float2(0.f, 0.f); }
                    const float mult = has_mirror ? 2.f : 1.f;
                    s_ww += mult * (w * w); s_wd += mult * (w * dw);
                }
            });
            if (tid == 0) { wtab[N / 2] = make_float2(1.f, 0.f); s_ww += 1.f; }
            if (p.normalize) {
                // time_frequency.py:25: w / sqrt(sum w^2) and the derivative of the quotient (fixed-order sums)
                s_ww = wave_sum(s_ww);
                s_wd = wave_sum(s_wd);
                __syncthreads();
                if (lane == 0) { red[wave] = s_ww; red[16 + wave] = s_wd; }
                __syncthreads();
                float ww = 0.f, wd = 0.f;
                for (int q = 0; q < WAVES; ++q) { ww += red[q]; wd += red[16 + q]; }
                __syncthreads();
                const float inv = 1.0f / sqrtf(ww);
                for (int n = tid; n < (WIN_SYM ? N / 2 + 1 : N); n += THREADS) {
                    const float2 e = wtab[n];
                    wtab[n] = make_float2(e.x * inv, e.y * inv - e.x * wd * inv * inv * inv);
                }
                if constexpr (TPW > 1) {
                    __syncthreads();
                    static_for<0, WPT>([&](auto ww_) {
                        constexpr int wi = decltype(ww_)::value;
                        const int n = tid + THREADS * wi;
                        if (n < N / 2) wkeep[wi] = wtab[n];
                    });
                    wmid = wtab[N / 2];
                }
            }
        }
        // ---- clip mean (models.py:38) --------------------------------------------------------------
        // the waves' sums meet in LDS (the barrier is also the window table's) and are added pairwise, in a fixed order; the quotient
        // by L is rounded once (dmel_kernels.h: "the clip mean")
        auto mean_of = [&](float wsum) -> float {
            if (lane == 0) red[wave] = wsum;
            __syncthreads();
            float t[WAVES];
            static_for<0, WAVES>([&](auto qq) { t[decltype(qq)::value] = red[decltype(qq)::value]; });
            static_for<0, ilog2(WAVES)>([&](auto ll) {
                constexpr int st = 1 << decltype(ll)::value;
                static_for<0, WAVES / (2 * st)>([&](auto ii) { constexpr int i = decltype(ii)::value * 2 * st; t[i] += t[i + st]; });
            });
            return mean_quotient(t[0], FWD_LC, FWD_INV_L);
        };
#ifdef DMEL_ABLATE
        const bool dbg_no_mean = (p.flags & 0x1000u) != 0;      // timing ablation: no clip sum (mean = 0)
#else
        constexpr bool dbg_no_mean = false;
#endif
        if (dbg_no_mean) {
            if constexpr (WIN_LDS) __syncthreads();
        } else if (WPF == 1 && p.remove_dc && p.psum == nullptr && p.tiles_per_clip == 1 && p.hop <= N / 2) {
            // The whole clip is this workgroup's: its frames already hold every sample -- frame t owns the hop segment
            // [t hop, (t + 1) hop) of the clip, which lies in its second half (hop <= N/2) -- so the clip is added up from the
            // registers the transform is about to use and never read a second time.  Fixed order: registers ascending inside a lane,
            // the 64 lanes by wave_sum, the waves ascending.
            float ps = 0.f;
            static_for<0, PASSES>([&](auto pp) {
                constexpr int pass = decltype(pp)::value;
                const int slot = pass * (WAVES * FPW) + wave * FPW + j;
                const int tA = PAIR ? 2 * slot : slot;                       // tile 0 of a one-tile clip: t0 = 0
                static_for<R / 2, R>([&](auto aa) {
                    constexpr int a = decltype(aa)::value;
                    const int n = lg + G * a;                                // >= N/2: inside the frame's second half
                    const bool seg = n < N / 2 + p.hop;
                    const int ia = tA * p.hop - N / 2 + n;
                    ps += (seg && tA < FWD_TC && ia < FWD_LC) ? xa[0][pass][a] : 0.f;
                    if constexpr (PAIR) ps += (seg && tA + 1 < FWD_TC && ia + p.hop < FWD_LC) ? xb2[0][pass][a] : 0.f;
                });
            });
            mean = mean_of(wave_sum(ps));
        } else if (p.remove_dc && p.psum == nullptr) {
            // short clips: every workgroup adds up its clip itself (L2 hits after the first toucher), in a
            // fixed order, instead of a separate pass over x
            // Loads go out in batches of 8 per thread before anything is added: one memory round trip per batch
            // instead of one per load (a plain loop waits for every load before issuing the next).
            const float* xc = xbase + (size_t)b * p.L;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int i = 0;
            constexpr int KB = 8;
            if ((reinterpret_cast<uintptr_t>(xc) & 15) == 0) {
                const float4* x4 = reinterpret_cast<const float4*>(xc);
#ifdef DMEL_ABLATE
                const int n4 = (p.flags & 0x40000u) ? p.L / 8 : ((p.flags & 0x80000u) ? p.L / 16 : p.L / 4);   // timing only: part of the clip
#else
                const int n4 = FWD_LC / 4;
#endif
                for (int base = 0; base < n4; base += THREADS * KB) {
                    float4 v[KB];
                    static_for<0, KB>([&](auto jj) {
                        constexpr int jv = decltype(jj)::value;
                        const int q = base + tid + THREADS * jv;
                        v[jv] = x4[q < n4 ? q : n4 - 1];
                    });
                    static_for<0, KB>([&](auto jj) {
                        constexpr int jv = decltype(jj)::value;
                        // (one select per 16-byte load instead of four: a + 1 v is a + v to the bit, a + 0 v is a -- the clamped load read a
                        // sample of this very clip, so a non-finite one is in the true sum too)
                        const float okf = (base + tid + THREADS * jv < n4) ? 1.f : 0.f;
                        a0 = fmaf(v[jv].x, okf, a0); a1 = fmaf(v[jv].y, okf, a1); a2 = fmaf(v[jv].z, okf, a2); a3 = fmaf(v[jv].w, okf, a3);
                    });
                }
                i = n4 * 4;
            }
            // what is left (the last L % 4 samples, or everything for a clip that is not 16-byte aligned): dword buffer
            // loads, out-of-range offsets return 0
            for (int base = i; base < FWD_LC; base += THREADS * KB) {
                float v[KB];
                static_for<0, KB>([&](auto jj) { v[decltype(jj)::value] = buf_f32(rx, (base + tid + THREADS * decltype(jj)::value) * 4); });
                static_for<0, KB>([&](auto jj) { a0 += v[decltype(jj)::value]; });
            }
            mean = mean_of(wave_sum((a0 + a1) + (a2 + a3)));
        } else {
            if constexpr (WIN_LDS) __syncthreads();              // window table complete
            if (p.remove_dc) {
                // long clips: the <= 64 partial sums of the prep kernel, one per lane, one round trip, added
                // in a fixed butterfly order (deterministic)
                mean = mean_quotient(wave_sum(ps_early), FWD_LC, FWD_INV_L);
            }
        }
        STAMP(2);   // window table + clip mean done
    }

    // kTrainH: PD[k] of a slot goes out as four bf16 values -- P hi, P lo, D hi, D lo, planes of NHS entries each: hi = bf16(v),
    // lo = bf16(v - hi), v = hi + lo to 2^-17 -- so that phase 2 reads its A operands (8 consecutive bins of one plane) with one
    // ds_read_b128 per lane and the three products hi hi + lo hi + hi lo stand for one fp32 product.
    auto store_h = [&](int slot_bytes, int k, v2f pdv) {
        const unsigned short ph = bf16_bits(pdv.x), dh = bf16_bits(pdv.y);
        const unsigned short pl = bf16_bits(pdv.x - __uint_as_float((unsigned)ph << 16)), dl = bf16_bits(pdv.y - __uint_as_float((unsigned)dh << 16));
        unsigned short* q = reinterpret_cast<unsigned short*>(smem_raw + slot_bytes) + k;
        q[0] = ph; q[NHS] = pl; q[2 * NHS] = dh; q[3 * NHS] = dl;
    };
    auto load_h = [&](int slot_bytes, int plane, int k) -> float {          // hi + lo of one bin of plane pair `plane` (0: P, 1: D)
        const unsigned short* q = reinterpret_cast<const unsigned short*>(smem_raw + slot_bytes) + 2 * plane * NHS + k;
        return __uint_as_float((unsigned)q[0] << 16) + __uint_as_float((unsigned)q[NHS] << 16);
    };

    // ================= the tiles of this workgroup ==============================================
    static_for<0, TPW>([&](auto tt) {
        constexpr int ti = decltype(tt)::value;
        if (ti > 0 && tile0 + ti >= p.tiles_per_clip) return;          // the clip has no such tile (same answer in every wave)
        const int t0 = (tile0 + ti) * FPT;
#if DMEL_FWD_LEN
        if (ti > 0 && t0 >= Tc) { fill_rows(t0, t0 + FPT, true); return; }      // a later tile past the clip: its pad rows only
#endif
        if constexpr (ti > 0) STAMP(16 * ti + 2);   // previous tile's epilogue issued, this tile begins
        if constexpr (ti > 0) {
            // the FFT slots (every wave has read the previous tile's spectra before the barriers of its phase 2 or the one
            // here) and the window table / half-tile exchange region are used again
            __syncthreads();
            // this tile's samples: requested here (behind the barrier, where the registers of the previous tile's matrix phase
            // are free; requested earlier they have to live through that phase and spill); the window rewrite covers part
            // of the round trip, and the lines were touched by the neighbouring frames before
            __builtin_amdgcn_sched_barrier(0);
            if (!dbg_skip_fft) load_tile(IC<ti>{});
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (WIN_ALIASED) {
                static_for<0, WPT>([&](auto ww_) {
                    constexpr int wi = decltype(ww_)::value;
                    const int n = tid + THREADS * wi;
                    if (n < N / 2) {
                        wtab[n] = wkeep[wi];
                        if constexpr (!WIN_SYM) { if (n > 0) wtab[N - n] = (p.win_half && n <= N / 4) ? make_float2(0.f, 0.f) : wkeep[wi]; }
                    }
                });
                if (tid == 0) wtab[N / 2] = wmid;
                __syncthreads();
            }
        }
        // ================= phase 1: FFT of this wave's frames ====================================
        if (!dbg_skip_fft) {
            static_for<0, PASSES>([&](auto pp) {
                constexpr int pass = decltype(pp)::value;
                const int slot = (WPF > 1) ? wave / WPF : pass * (WAVES * FPW) + wave * FPW + j;
                v2f* sl = lds + slot * SS;
                const int tA = PAIR ? (t0 + 2 * slot) : (t0 + slot);
                const int f0 = tA * p.hop - N / 2;                       // first sample of frame tA
                const int f1 = PAIR ? f0 + p.hop : f0;
                // zero padding of torch.stft(center=True, pad_mode='constant') applies AFTER the DC removal
                bool inside_w = inside[ti][pass];
#ifdef DMEL_ABLATE
                if (p.flags & 0x20000u) inside_w = true;          // timing only: clamped loads kept, no selects
#endif
                v2f z[R];
                // window entries of this lane: one base register + compile-time offsets (ds_read_b64 offset:512a)
                int wbyte = (WIN_LDS ? g.AUX_OFF : 0) + lg * 8;
                int wbyte_m = g.AUX_OFF + (G - lg) * 8;                      // half table: entry N - n of n = lg + G a, a >= R/2
                asm volatile("" : "+v"(wbyte), "+v"(wbyte_m));
                auto wload = [&](auto aa_) -> v2f {
                    constexpr int a = decltype(aa_)::value;
                    float2 wd2;                                              // (w[n], dw[n] / d|lambd| * scale)
                    if constexpr (WIN_SYM && a >= R / 2) {
                        wd2 = *reinterpret_cast<const float2*>(smem_raw + wbyte_m + G * 8 * (R - 1 - a));
                        // the half-length window of torch.stft covers [N/4, 3N/4): entry 3N/4 is zero, its mirror image is not
                        if constexpr (a == 3 * R / 4) { if (p.win_half && lg == 0) wd2 = make_float2(0.f, 0.f); }
                    }
                    else if constexpr (WIN_LDS) wd2 = *reinterpret_cast<const float2*>(smem_raw + wbyte + G * 8 * a);
                    else wd2 = *reinterpret_cast<const float2*>(reinterpret_cast<const unsigned char*>(FWD_WIN2) + wbyte + G * 8 * a);
                    return v2f{wd2.x, wd2.y};
                };
#ifdef DMEL_ABLATE
                // timing only (VERDICT r05 #1, upper bound): the frames lose a mean the wave adds up from its own samples, and what is left of the
                // clip mean is applied in the pairing pass as a frequency-domain correction (a table read + one packed FMA per bin pair)
                float mean_w = mean;
                if (p.flags & 0x200000u) {
                    float sm_loc = 0.f;
                    static_for<0, R>([&](auto aa) { sm_loc += xa[ti][pass][decltype(aa)::value]; });
                    mean_w = wave_sum(sm_loc) * (1.0f / (64.f * R));
                }
                const float dlt_late = mean - mean_w;
#define DMEL_MEAN_W mean_w
#else
#define DMEL_MEAN_W mean
#endif
                // (every mode but the wave-local one, R = 32 or 64: the window multiply in groups of eight entries -- left alone the scheduler requested
                // all R window entries at once, R register pairs on top of the R samples and the growing z, and spilled 6 ... 22 registers at
                // n_fft 1024 ... 4096 (tools/kres.sh; VERDICT r05 #4); kTrainW fits as it is and is not touched)
#ifndef DMEL_WIN_GROUP
#define DMEL_WIN_GROUP 8
#endif
                constexpr bool WIN_GROUPED = !WLC && R >= 32 && DMEL_WIN_GROUP > 0;
                if (inside_w) {
                    float mean_i = DMEL_MEAN_W;
                    if constexpr (WIN_GROUPED) asm volatile("" : "+v"(mean_i));      // (its own copy: the R subtractions are then not hoisted above the branch as one block)
                    static_for<0, R>([&](auto aa) {
                        constexpr int a = decltype(aa)::value;
                        if constexpr (WIN_GROUPED && a % (DMEL_WIN_GROUP > 0 ? DMEL_WIN_GROUP : 1) == 0 && a > 0) __builtin_amdgcn_sched_barrier(0);
                        const v2f wd = wload(aa);
                        const float va = xa[ti][pass][a] - mean_i;
                        if constexpr (!PAIR) z[a] = splat(va) * wd;
                        else z[a] = v2f{va, xb2[ti][pass][a] - mean_i} * wd.xx;
                    });
                } else {
#if DMEL_FWD_LEN
                    // samples of the clip only; a pad frame (Tc <= t < T) is all zero: its spectrum, mel power and tangent are exactly 0.  Frames
                    // past the output (t >= T, never written) keep the default path's samples: the pair modes' two frames of a complex FFT share
                    // its rounding, and with Lc = L every frame must come out as dmel_fwd_kernel's
#if DMEL_FWD_FB
                    // (kSpec of a trained bank's build: the filterbank gradient never loads the column of a pad frame, so such a frame keeps the
                    // clip's samples it overlaps -- one uniform bound, as dmel_fwd_kernel's p.L, instead of two per lane: at n_fft 2048 ... 8192 the
                    // per-lane bounds cost 4 ... 6 spilled registers more than dmel_fwd_kernel's kSpec)
                    const int lim_a = (IS_SPEC || tA < Tc || tA >= p.T) ? Lc : 0;
                    [[maybe_unused]] const int lim_b = (IS_SPEC || tA + 1 < Tc || tA + 1 >= p.T) ? Lc : 0;
#else
                    const int lim_a = (tA < Tc || tA >= p.T) ? Lc : 0;
                    [[maybe_unused]] const int lim_b = (tA + 1 < Tc || tA + 1 >= p.T) ? Lc : 0;
#endif
#define FWD_LIM_A lim_a
#define FWD_LIM_B lim_b
#else
#define FWD_LIM_A p.L
#define FWD_LIM_B p.L
#endif
                    static_for<0, R>([&](auto aa) {
                        constexpr int a = decltype(aa)::value;
                        const int n = lg + G * a;
                        const v2f wd = wload(aa);
                        const int ia = f0 + n;
                        const float va = ((ia >= 0) && (ia < FWD_LIM_A)) ? xa[ti][pass][a] - mean : 0.f;
                        if constexpr (!PAIR) z[a] = splat(va) * wd;
                        else {
                            const int ib = f1 + n;
                            const float vb = ((ib >= 0) && (ib < FWD_LIM_B)) ? xb2[ti][pass][a] - mean : 0.f;
                            z[a] = v2f{va, vb} * wd.xx;
                            // (the frames at a clip's edge, pair modes: four entries at a time.  Interleaved freely, the index arithmetic of all R entries
                            // raised this RARE path's register demand past the budget, and what it spilled -- z[0 .. 4] -- was spilled on the interior path too)
                            if constexpr (WIN_GROUPED && a % 4 == 3) __builtin_amdgcn_sched_barrier(0);
                        }
                    });
                }
#if DMEL_FWD_LEN
                // (radix-8 and radix-4 plans, n_fft 32 ... 128: the windowed samples are materialised before the transform.  Without this the
                // backend fused two window products into the first butterflies (two v_pk_mul_f32 + v_pk_add_f32 became v_pk_fma_f32), which
                // dmel_fwd_kernel does not: full-length clips came out 1 - 2 ulp off the default path.  With it both round alike.)
                // (kSpec of a trained bank's build, DMEL_FWD_FB: not there -- dmel_fwd_kernel's kSpec does fuse them)
#if DMEL_FWD_FB
                if constexpr (R <= 8 && !IS_SPEC) {
#else
                if constexpr (R <= 8) {
#endif
#pragma unroll
                    for (int a = 0; a < R; ++a) asm volatile("" : "+v"(z[a]));
                }
#endif
                STAMP(16 * ti + 3);   // samples arrived, windowed
                if constexpr (USE_DIT) fft_reg_dit<R>(z); else fft_reg<R>(z);
                STAMP(16 * ti + 4);   // radix-R #1
                // twiddle w_N^(lg*q), transposition through LDS: S[q][lg]
                v2f u[R];
                // The R - 1 twiddles w^q (w = w_N^lg) of a lane are N*8 bytes of table per frame (32 KB at n_fft 4096).  With TW1_POW
                // only rows q = 1 and q = 8a are loaded, w^(8a+b) = w^(8a) w^b with w^2..w^7 by repeated multiplication (<= 7
                // roundings: ~5e-7 relative, the transform's own noise): R/8 loads and about R complex products instead of R - 1 loads.
                // Measured: config 2 21.87 -> 21.52 us, config 3 49.7 -> 47.4, config 5 74.3 -> 71.9, ESC-50 shape 164 -> 157 (n_fft 4096)
                // and 514 -> 485 (8192); errors against the fp64 oracle unchanged (3e-7 of the loudest bin).  The two or four rows are
                // requested HERE: asked for at the top of the kernel (8 more live registers through the prologue) the 32 x 32 plan measured
                // 22.0 us against 20.0 at config 2, copied to LDS once per workgroup 20.2 against 19.7
                v2f wb[TW1_POW ? 8 : 1];
                if constexpr (TW1_POW) {
                    const float2 w1 = p.tw1[G + lg];
                    wb[1] = v2f{w1.x, w1.y};
                    static_for<2, 8>([&](auto bb) { constexpr int b = decltype(bb)::value; wb[b] = cmul(wb[b - 1], w1); });
                }
                int tw1b = g.TW1_OFF + lg * 8;                               // one base register, compile-time offsets (ds_read_b64 offset: 8 G (q - 1))
                asm volatile("" : "+v"(tw1b));
                auto twiddled = [&](auto qq, v2f v) -> v2f {
                    constexpr int q = decltype(qq)::value;
                    if constexpr (q == 0) return v;
                    else if constexpr (TW1_LDS) return cmul(v, *reinterpret_cast<const float2*>(smem_raw + tw1b + (q - 1) * (G * 8)));
                    else if constexpr (!TW1_POW) return cmul(v, p.tw1[q * G + lg]);
                    else {
                        constexpr int a8 = q / 8, b8 = q % 8;
                        if constexpr (a8 == 0) return cmul(v, float2{wb[b8].x, wb[b8].y});
                        else {
                            const float2 anchor = p.tw1[(8 * a8) * G + lg];
                            if constexpr (b8 == 0) return cmul(v, anchor);
                            else { const v2f t = cmul(wb[b8], anchor); return cmul(v, float2{t.x, t.y}); }
                        }
                    }
                };
                if constexpr (!SPLIT) {
                    static_for<0, R>([&](auto qq) {
                        constexpr int q = decltype(qq)::value;
                        sl[q * EXS + lg] = twiddled(qq, z[bitrev(q, LB)]);
                    });
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    static_for<0, R>([&](auto bb) {
                        constexpr int bi = decltype(bb)::value;
                        u[bi] = sl[qp * EXS + r + C * bi];
                    });
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                } else {
                    // one plane of N floats: real parts through, then imaginary parts (LDS executes a wave's accesses in order, so
                    // the second set of writes cannot overtake the first set of reads)
                    float* slf = reinterpret_cast<float*>(sl);
#ifndef DMEL_TW1_CHUNK
#define DMEL_TW1_CHUNK 4
#endif
                    // first-stage twiddles from the LDS table in chunks, the next chunk requested while one is used (as the radix-C twiddles
                    // below): read one by one, every element waited for its own LDS round trip behind the plane write of the one before
                    // (`ds_read_b64; s_waitcnt lgkmcnt(0)` 31 times per wave in the assembly).  Chunks of 4 or 8: config 4's batch 106.9-107.0 -> 105.9-106.2 us, config 2
                    // within the noise; chunks of 16 spill (+4.5 %)
                    constexpr int TW1C = (TW1_LDS && DMEL_TW1_CHUNK > 0) ? DMEL_TW1_CHUNK : R;
                    float2 tw1r[(TW1_LDS && DMEL_TW1_CHUNK > 0) ? R : 1];
                    auto tw1_fetch = [&](auto cc) {
                        constexpr int c0 = decltype(cc)::value;
                        static_for<(c0 == 0 ? 1 : c0), (c0 + TW1C < R ? c0 + TW1C : R)>([&](auto q1) {
                            constexpr int q = decltype(q1)::value;
                            tw1r[q] = *reinterpret_cast<const float2*>(smem_raw + tw1b + (q - 1) * (G * 8));
                        });
                    };
                    if constexpr (TW1_LDS && DMEL_TW1_CHUNK > 0) {
                        tw1_fetch(IC<0>{});
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    static_for<0, R>([&](auto qq) {
                        constexpr int q = decltype(qq)::value;
                        v2f v;
                        if constexpr (TW1_LDS && DMEL_TW1_CHUNK > 0) {
                            if constexpr (q % TW1C == 0 && q + TW1C < R) {
                                __builtin_amdgcn_sched_barrier(0);
                                tw1_fetch(IC<q + TW1C>{});
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            v = z[bitrev(q, LB)];
                            if constexpr (q != 0) v = cmul(v, tw1r[q]);
                        } else v = twiddled(qq, z[bitrev(q, LB)]);
                        z[bitrev(q, LB)] = v;
                        slf[q * EXS + lg] = v.x;
                    });
                    sync_frame();
                    float ure[R];
                    static_for<0, R>([&](auto bb) {
                        constexpr int bi = decltype(bb)::value;
                        ure[bi] = slf[qp * EXS + r + C * bi];
                    });
                    sync_frame();
                    static_for<0, R>([&](auto qq) {
                        constexpr int q = decltype(qq)::value;
                        slf[q * EXS + lg] = z[bitrev(q, LB)].y;
                    });
                    sync_frame();
                    static_for<0, R>([&](auto bb) {
                        constexpr int bi = decltype(bb)::value;
                        u[bi] = v2f{ure[bi], slf[qp * EXS + r + C * bi]};
                    });
                    sync_frame();
                }
                STAMP(16 * ti + 5);   // twiddle + LDS transposition
                // the radix-C twiddles w_G^(r*p1) are requested before the second radix-R stage, not one by one inside the
                // cross-lane stage (each read there was waited for on the spot)
                // (R = 32: in chunks of 8, the next chunk requested while one is used -- all 31 at once cost 62 registers on top of
                // the 64 of the transform)
                constexpr int TWC = (R > 16) ? DMEL_TWC : R;
                float2 tw2r[R];
                auto tw2_fetch = [&](auto cc) {
                    constexpr int c0 = decltype(cc)::value;
                    static_for<(c0 == 0 ? 1 : c0), (c0 + TWC < R ? c0 + TWC : R)>([&](auto pp1) {
                        constexpr int p1 = decltype(pp1)::value;
                        if constexpr (TW2_LDS) tw2r[p1] = tw2l[p1 * C + r]; else tw2r[p1] = p.tw2[p1 * C + r];
                    });
                };
                if constexpr (C > 1) {
                    tw2_fetch(IC<0>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (USE_DIT) fft_reg_dit<R>(u); else fft_reg<R>(u);
                STAMP(16 * ti + 6);   // radix-R #2
                // twiddle w_G^(r*p1), radix-C across adjacent lanes, spectrum to LDS in natural order
                const v2f rot_f = splat((C == 4 && r == 3) ? 0.f : 1.f);
                const v2f rot_e = (C == 4 && r == 3) ? v2f{1.f, -1.f} : v2f{0.f, 0.f};
                v2f zr[KEEPZ ? R : 1];                                   // Z[qp + R p1 + R R p2] of this lane, by p1
                static_for<0, R>([&](auto pp1) {
                    constexpr int p1 = decltype(pp1)::value;
                    if constexpr (C > 1 && TWC < R && p1 % TWC == 0 && p1 + TWC < R) {
                        __builtin_amdgcn_sched_barrier(0);
                        tw2_fetch(IC<p1 + TWC>{});
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    v2f v = u[bitrev(p1, LB)];
                    int p2 = 0;
                    if constexpr (C > 1) {
                        if constexpr (p1 != 0) v = cmul(v, tw2r[p1]);
                    }
                    if constexpr (C == 2) {
                        const v2f o = v2f{quad_xor1(v.x), quad_xor1(v.y)};
                        v = __builtin_elementwise_fma(splat((r == 0) ? 1.f : -1.f), v, o);
                        p2 = r;
                    } else if constexpr (C == 4) {
                        v2f o = v2f{quad_xor2(v.x), quad_xor2(v.y)};
                        v2f t = __builtin_elementwise_fma(splat((r < 2) ? 1.f : -1.f), v, o);
                        t = __builtin_elementwise_fma(t.yx, rot_e, t * rot_f);      // lane r == 3: t * (-i); others: t
                        o = v2f{quad_xor1(t.x), quad_xor1(t.y)};
                        v = __builtin_elementwise_fma(splat(((r & 1) == 0) ? 1.f : -1.f), t, o);
                        p2 = ((r & 1) << 1) | (r >> 1);
                    }
                    if constexpr (KEEPZ) zr[p1] = v;
                    else {
                        const int k = qp + R * p1 + R * R * p2;
                        sl[z_index<R, C>(k)] = v;
                    }
                });
                if constexpr (KEEPZ) {
                    // ---- pairing pass without the spectrum in LDS.  Z[N-k] of k = qp + R p1 + R^2 p2 is Z[qp' + R p1' + R^2 p2'] with
                    //   qp > 0:            qp' = R - qp, p1' = R - 1 - p1,  p2' = C - 1 - p2
                    //   qp = 0, p1 > 0:    qp' = 0,      p1' = R - p1,      p2' = C - 1 - p2
                    //   qp = 0, p1 = 0:    qp' = 0,      p1' = 0,           p2' = (C - p2) mod C
                    // i.e. one fixed partner lane (two for the four lanes with qp = 0) and a register index that depends on p1 only:
                    // each lane offers the register its partner wants (a select between the two cases) and ds_bpermute_b32 hands
                    // it over -- LDS crossbar, no LDS storage.  Rounds p1 < R/2 meet every pair {k, N-k} exactly once (the partner
                    // register is >= R/2), one more round covers p1 = R/2 on the qp = 0 lanes.  PD is symmetric in k <-> N-k, so
                    // the lane that holds the upper bin writes PD[N-k]; only PD[0..N/2] exists in LDS, over the transposition plane.
                    constexpr int PADC = (C > 1) ? 4 : 0, RR = R * R;
                    auto lane_of_p2 = [](int v) { return C == 4 ? (((v & 1) << 1) | (v >> 1)) : v; };
                    const int p2 = lane_of_p2(r);                              // (the digit reversal is its own inverse)
                    const bool q0 = (qp == 0);
                    const bool dir_a = (2 * p2 < C);                             // this lane's bins are <= N/2: it writes PD[k], else PD[N-k]
                    const int p2m = C - 1 - p2;
                    const int fl0 = j * G;                                      // first lane of this frame inside the wave (G < 64: FPW frames)
                    const int pull1 = (fl0 + ((R - qp) & (R - 1)) * C + lane_of_p2(p2m)) * 4;
                    const int pull0 = q0 ? (fl0 + lane_of_p2((C - p2) % C)) * 4 : pull1;
                    // PLANE (frames of several waves): the partner lane may sit in another wave, so Z[N-k] goes through one plane
                    // of floats in the frame's slot, indexed k + PLANE_PAD (k / R^2): real parts written, read mirrored, then the
                    // imaginary parts through the same plane.  Mirror index of (qp, p1, p2): the partner's own index, linear in p1.
                    constexpr int PP = g.PLANE_PAD;
                    float* plane = reinterpret_cast<float*>(sl);
                    const int pidx = qp + (RR + PP) * p2;                              // + R p1
                    const int midx = (R - qp) + R * (R - 1) + (RR + PP) * p2m;         // - R p1   (qp = 0: R - qp = R, no wrap)
                    const int midx0 = q0 ? (RR + PP) * ((C - p2) % C) : midx;         // p1 = 0
                    float znx[PLANE ? R / 2 + 1 : 1];
                    if constexpr (PLANE) {
                        static_for<0, R>([&](auto pp1) { constexpr int p1 = decltype(pp1)::value; plane[pidx + R * p1] = zr[p1].x; });
                        sync_frame();
                        static_for<0, R / 2 + 1>([&](auto pp1) {
                            constexpr int p1 = decltype(pp1)::value;
                            znx[p1] = plane[(p1 == 0) ? midx0 : midx - R * p1];
                        });
                        sync_frame();
                        static_for<0, R>([&](auto pp1) { constexpr int p1 = decltype(pp1)::value; plane[pidx + R * p1] = zr[p1].y; });
                        sync_frame();
                    }
                    v2f pdk[PLANE ? R / 2 + 1 : 1];                                    // PLANE: PD overwrites the plane, after everyone has read it
                    const int slot_b = slot * (SS * 8);
                    const int base_a = slot_b + (qp + (RR + PADC) * p2) * 8;
                    const int base_b = slot_b + ((R - qp) + R * (R - 1) + (RR + PADC) * p2m) * 8;
                    const int obase = dir_a ? base_a : base_b;
                    const int ostep = dir_a ? R * 8 : -R * 8;
                    const bool nyq = q0 && (2 * p2 == C);                        // k = N/2 (C > 1: round 0; C = 1: the extra round)
                    // (kTrainW reads PD[k] at 8 k for every k <= N/2: its Nyquist bin sits at the unpadded position)
                    const int addr0 = nyq ? slot_b + (N / 2 + (WLC ? 0 : PADC * (C / 2))) * 8 : obase;
                    const bool w0 = dir_a || !q0 || nyq;
                    static_for<0, R / 2 + 1>([&](auto pp1) {
                        constexpr int p1 = decltype(pp1)::value;
                        constexpr int s_a = (p1 == R / 2) ? R / 2 : (R - 1 - p1);        // what a partner with qp > 0 wants
                        constexpr int s_b = (p1 == R / 2) ? R / 2 : ((R - p1) % R);      // ... with qp = 0
                        // (component by component: a scalar-condition select of two ext vectors lost its second lane here)
                        const float send_x = (s_a == s_b) ? zr[s_a].x : (q0 ? zr[s_b].x : zr[s_a].x);
                        const float send_y = (s_a == s_b) ? zr[s_a].y : (q0 ? zr[s_b].y : zr[s_a].y);
                        v2f zn;
                        if constexpr (PLANE) {
                            zn = v2f{znx[p1], plane[(p1 == 0) ? midx0 : midx - R * p1]};
                        } else {
                            const int pull = (p1 == 0) ? pull0 : pull1;
                            const int got_x = __builtin_amdgcn_ds_bpermute(pull, __builtin_bit_cast(int, send_x));
                            const int got_y = __builtin_amdgcn_ds_bpermute(pull, __builtin_bit_cast(int, send_y));
                            zn = v2f{__builtin_bit_cast(float, got_x), __builtin_bit_cast(float, got_y)};
                        }
                        const v2f zk = zr[p1];
                        float sx = zk.x + zn.x, sy = zk.y - zn.y, dx = zk.x - zn.x, dy = zk.y + zn.y;
#ifdef DMEL_ABLATE
                        if constexpr (WIN_LDS) {
                            if (p.flags & 0x200000u) {          // timing only: stand-in for (2 W[k], 2 W'[k]) of the window's own transform
                                const float2 cw = *reinterpret_cast<const float2*>(smem_raw + wbyte + G * 8 * (p1 % (R / 2)));
                                sx = fmaf(-dlt_late, cw.x, sx); dy = fmaf(-dlt_late, cw.y, dy);
                            }
                        }
#endif
                        v2f pdv;
                        if constexpr (!PAIR) pdv = v2f{fmaf(sx, sx, sy * sy), fmaf(sx, dy, -(sy * dx))};
                        else pdv = v2f{fmaf(sx, sx, sy * sy), fmaf(dx, dx, dy * dy)};
                        if constexpr (PLANE) pdk[p1] = pdv;
                        else if constexpr (HSPLIT) {
                            // the same bins, unpadded, into the bf16 planes of the slot
                            const int kb_a = qp + RR * p2, kb_b = (R - qp) + R * (R - 1) + RR * p2m;
                            const int kb0 = dir_a ? kb_a : kb_b, kbs = dir_a ? R : -R;
                            if constexpr (p1 == 0) { if (w0) store_h(slot_b, nyq ? N / 2 : kb0, pdv); }
                            else if constexpr (p1 < R / 2) store_h(slot_b, kb0 + kbs * p1, pdv);
                            else { if (q0 && dir_a) store_h(slot_b, kb_a + R * (R / 2), pdv); }
                        }
                        else if constexpr (p1 == 0) { if (w0) *reinterpret_cast<v2f*>(smem_raw + addr0) = pdv; }
                        else if constexpr (p1 < R / 2) *reinterpret_cast<v2f*>(smem_raw + obase + ostep * p1) = pdv;
                        else { if (q0 && dir_a) *reinterpret_cast<v2f*>(smem_raw + base_a + R * 8 * (R / 2)) = pdv; }
                    });
                    if constexpr (PLANE) {
                        sync_frame();
                        static_for<0, R / 2 + 1>([&](auto pp1) {
                            constexpr int p1 = decltype(pp1)::value;
                            if constexpr (p1 == 0) { if (w0) *reinterpret_cast<v2f*>(smem_raw + addr0) = pdk[p1]; }
                            else if constexpr (p1 < R / 2) *reinterpret_cast<v2f*>(smem_raw + obase + ostep * p1) = pdk[p1];
                            else { if (q0 && dir_a) *reinterpret_cast<v2f*>(smem_raw + base_a + R * 8 * (R / 2)) = pdk[p1]; }
                        });
                    }
                    // the filterbank fragments of phase 2: requested once the spectrum registers are dead
                    if constexpr (pass == PASSES - 1) { __builtin_amdgcn_sched_barrier(0); fetch_bpre(); wl_prefetch(); }
                } else {
                // the filterbank fragments of phase 2 are requested here: the registers of the FFT are free, and the pairing
                // pass plus the barrier behind it cover the round trip
                if constexpr (pass == PASSES - 1) { fetch_bpre(); __builtin_amdgcn_sched_barrier(0); }
                // ---- pairing pass: the two real spectra packed in Z are separated ONCE per bin here, by the wave
                // that owns the slot, instead of by every A-fragment builder in phase 2:
                //   S = Z[k] + conj Z[N-k], D = Z[k] - conj Z[N-k];  PD[k] = (|S|^2, Im(conj S * D))   (train: 4|X|^2, 2 d|X|^2)
                //                                                    PD[k] = (|S|^2, |D|^2)           (pairs: 4|Xa|^2, 4|Xb|^2)
                // stored in place over Z[0 .. N/2] (all reads of the wave precede its writes: LDS is in order per wave)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                constexpr int NPAIR = N / (2 * G) + 1;           // bins lg + G*i <= N/2
                // Addresses are one of four per-lane byte bases plus a compile-time offset (ds_read_b64 offset:...):
                //   Z[k],   k = lg + G i:            zb + 8 (G i + pad(G i))
                //   Z[N-k], lg >= 1:                 mb + 8 (c_i + pad(c_i)),  mb = slot + 8 (G - lg),  c_i = N - G (i + 1)
                //   lane 0: N - G i itself; it sits one padding step further when it starts an R*R block (mbA), and
                //   wraps to bin 0 for i = 0 (mb0).
                constexpr int PADC = (C > 1) ? 4 : 0, RR = R * R;
                const int slot_b = slot * (SS * 8);
                int zb = slot_b + lg * 8;
                int mb = slot_b + (G - lg) * 8;
                int mbA = mb + ((lg == 0) ? PADC * 8 : 0);
                int mb0 = (lg == 0) ? slot_b : mb + (N - G + PADC * ((N - G) / RR)) * 8;       // full address of Z[N-k] for i = 0
                asm volatile("" : "+v"(zb), "+v"(mb), "+v"(mbA), "+v"(mb0));
                v2f pd[NPAIR];
                static_for<0, NPAIR>([&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    constexpr int ck = G * i, cm = N - G * (i + 1);
                    constexpr bool crossing = PADC != 0 && ((N - G * i) % RR) == 0;
                    const int mbase = (i == 0) ? mb0 : (crossing ? mbA : mb);
                    const v2f zk = *reinterpret_cast<const v2f*>(smem_raw + zb + (ck + PADC * (ck / RR)) * 8);
                    const v2f zn = *reinterpret_cast<const v2f*>(smem_raw + mbase + ((i == 0) ? 0 : (cm + PADC * (cm / RR)) * 8));
                    const float sx = zk.x + zn.x, sy = zk.y - zn.y, dx = zk.x - zn.x, dy = zk.y + zn.y;
                    if constexpr (!PAIR) pd[i] = v2f{fmaf(sx, sx, sy * sy), fmaf(sx, dy, -(sy * dx))};
                    else pd[i] = v2f{fmaf(sx, sx, sy * sy), fmaf(dx, dx, dy * dy)};
                });
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                static_for<0, NPAIR>([&](auto ii) {
                    constexpr int i = decltype(ii)::value;
                    constexpr int ck = G * i;
                    v2f* dst = reinterpret_cast<v2f*>(smem_raw + zb + (ck + PADC * (ck / RR)) * 8);
                    if constexpr (HSPLIT) { if (i < NPAIR - 1 || lg == 0) store_h(slot_b, lg + ck, pd[i]); }
                    else
                    if (i < NPAIR - 1 || lg == 0) *dst = pd[i];          // the last round holds only the Nyquist bin
                });
                }
            });
        }
        STAMP(16 * ti + 7);   // twiddle + cross-lane radix-C + spectrum to LDS + pairing pass
        if constexpr (WLC) {
            // every wave goes on with the frames it transformed itself: its own LDS writes are all it waits for
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (p.spec_out) __syncthreads();          // (the saved spectrogram is written by all threads from all slots)
        } else __syncthreads();
        STAMP(16 * ti + 8);   // barrier
#ifdef DMEL_ABLATE
        if (dbg_skip_gemm) { if (tid == 0 && lds[0].x == 12345.678f) p.out[0] = 0.f; return; }
#endif
        float htan = 0.f;
        if constexpr (TRAINLIKE || MODE == kSpecTrain) htan = red[kRedTan];       // see the prologue
        if constexpr (TRAINLIKE) {
            // a trainable filterbank's gradient contracts this very spectrogram with the output's gradient (models.py:53): written out
            // here, (B, F, T) as time_frequency.py:53 lays it out, it saves dmel_backward_fb the recompute.  16 consecutive threads
            // write 16 consecutive frames of one bin: 64-byte pieces.
            if (p.spec_out) {
                for (int idx = tid; idx < SLOTS * F; idx += THREADS) {
                    const int k = idx / SLOTS, slot = idx % SLOTS;
                    const int t = t0 + slot;
                    if constexpr (HSPLIT) { if (t < p.T) p.spec_out[((size_t)b * F + k) * p.T + t] = 0.25f * load_h(slot * (SS * 8), 0, k); }
                    else
                    if (t < p.T) p.spec_out[((size_t)b * F + k) * p.T + t] = 0.25f * (lds + slot * SS)[WLC ? k : z_index<R, C>(k)].x;
                }
            }
        }
        if constexpr (IS_SPEC) {
            // power spectrogram (time_frequency.py:53), layout (B, F, T); kSpecTrain also writes d P / d lambd
            for (int idx = tid; idx < SLOTS * F; idx += THREADS) {
                const int k = idx / SLOTS, slot = idx % SLOTS;
                const v2f pdv = (lds + slot * SS)[z_index<R, C>(k)];
                if constexpr (MODE == kSpec) {
                    const int t = t0 + 2 * slot;
                    float* o = p.out + ((size_t)b * F + k) * p.T;
                    if (t < p.T) o[t] = 0.25f * pdv.x;
                    if (t + 1 < p.T) o[t + 1] = 0.25f * pdv.y;
                } else {
                    const int t = t0 + slot;
                    if (t < p.T) {
                        const size_t o = ((size_t)b * F + k) * p.T + t;
                        p.out[o] = 0.25f * pdv.x;
                        if (p.tangent) p.tangent[o] = htan * pdv.y;
                    }
                }
            }
        } else if constexpr (WLC) {
            // ================= phase 2, wave-local: v_mfma_f32_4x4x1_16b_f32 ==========================
            // One instruction multiplies 16 independent (4 x 1) (1 x 4) blocks.  Block b works for one quad of mel bands; its four
            // rows are this wave's (frame, P | D) pairs -- two frames of a 32-lane plan, or one frame (rows 2, 3 repeat 0, 1 and are
            // dropped) -- and a step feeds it ONE bin: lane 4 b + i supplies PD of row i at the block's current bin (one ds_read_b32,
            // consecutive steps are consecutive bins: immediate offsets), lane 4 b + j the filterbank coefficient of column j (four
            // steps per 16-byte load of a table every wave of the grid shares).  The HTK bank has at most two non-zeros per bin: a
            // quad's band is 5 .. 66 bins wide at n_fft 1024 and the 16 blocks of a phase (quads of similar width) walk their bands in
            // lock step -- 88 eight-cycle instructions per wave against 39 of 32 cycles for the banded 16 x 16 x 4 tiles, no workgroup
            // barrier in front (a wave needs nobody else's frames), no exchange of partial sums, the same work in every wave.
            const bool do_log = (p.flags & 1u) != 0;
            const bool out_bf16 = (p.flags & 4u) != 0;
            const int row = lane & 3;
            const int fr = (FPW == 2) ? (row & 1) : 0, typ = (FPW == 2) ? (row >> 1) : (row & 1);
            const int a_lane = (wave * FPW + fr) * (SS * 8) + typ * 4;
            const int tA = t0 + wave * FPW;                                    // first frame of this wave
            int off4 = 0;
            // one 64-bit base per tensor and clip in scalar registers, 32-bit element offsets per lane (M T < 2^31)
            float* const out_clip = p.out + (size_t)FWD_BO * p.M * p.T;
            unsigned short* const outh_clip = reinterpret_cast<unsigned short*>(p.out) + (size_t)FWD_BO * p.M * p.T;
            float* const tan_clip = p.tangent ? p.tangent + (size_t)FWD_BO * p.M * p.T : nullptr;
            // Staged epilogue (two phases at most -- 128 mel bands --, fp32 output, rows of whole 16-byte pieces): a lane's results --
            // 8 bytes per tensor and mel band, 64 different rows per store instruction -- are kept until the wave's last phase, written
            // over the wave's OWN frame slots (its spectra are dead by then), and after ONE workgroup barrier every thread stores
            // 16 bytes of a row: 4 lanes cover the tile's 16 frames of one (tensor, mel band), 64 contiguous bytes.  Measured with the
            // store pattern alone (tools/xtime.py 0x20000): config 2 18.8 -> 17.0 us, config 4's batch 117.7 -> 108.2 -- the scattered
            // 8-byte stores cost the memory pipeline a request per lane.
#ifndef DMEL_WL_STAGE
#define DMEL_WL_STAGE 1
#endif
            constexpr int NST = (FPW == 1) ? 4 : 2;                              // phases whose results a lane can keep (2 FPW values each)
            const bool staged = DMEL_WL_STAGE && p.wl_phases <= NST && p.M <= SS && !out_bf16 && (p.T & 3) == 0 && p.tangent != nullptr && SLOTS % 4 == 0;
            float sv[NST][2 * FPW];
            int sm[NST];
            static_for<0, NST>([&](auto pp) { sm[decltype(pp)::value] = -1; });
            // the lane table (and merge table) of phase ph + 1 is requested at the top of phase ph: asked for where it is used, every phase
            // began with a global round trip (~700 cycles: a phase cost as much as ~36 of its steps, which is what kept config 3's split
            // schedule -- three phases of 100 steps against two of 136 -- from paying)
            int2 li_pref = (WL_EARLY >= 1) ? wl_li[0] : p.wl_lane[lane];
            int mi_pref = (FPW == 1 && p.wl_mg[0] != 0) ? p.wl_merge[lane] : 0;
            for (int ph = 0; ph < p.wl_phases; ++ph) {
                const int n4 = p.wl_len4[ph];
                const int2 li = li_pref;
#if DMEL_FWD_BAND
                // a lane keeps its column only if the mel band is one of this channel's rows; a phase none of whose quads holds such a
                // band (the quads are sorted by width: the narrow low bands and the wide high ones sit in different phases) runs no steps
                const bool row_mine = li.y >= e_lo && li.y < e_hi;
                const int n4r = (!DMEL_BAND_SKIP || __any(row_mine)) ? n4 : 0;
#else
                const int n4r = n4;
#endif
                const int mi = mi_pref;
                if (ph + 1 < p.wl_phases) {
                    li_pref = p.wl_lane[(ph + 1) * 64 + lane];
                    if constexpr (FPW == 1) mi_pref = (p.wl_mg[ph + 1] != 0) ? p.wl_merge[(ph + 1) * 64 + lane] : 0;
                }
                if ((WL_EARLY < 2 && ph == 0) || (!DMEL_WL_NEXT && ph > 0)) wl_ring_init(n4, off4);      // (off4: still this phase's first group)
                off4 += n4;
                int aaddr = a_lane + li.x;
                floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                // A operands: the next group's four bins are requested before this group's MFMAs are issued (reads past the end of a
                // phase land on finite data of the slot and are not used).  B operands: the ring (see wl_bload).
                float a_cur[4];
                static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; a_cur[u] = *reinterpret_cast<const float*>(smem_raw + aaddr + 8 * u); });
                auto group = [&](auto dd) {
                    constexpr int d = decltype(dd)::value;
                    float a_nxt[4];
                    static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; a_nxt[u] = *reinterpret_cast<const float*>(smem_raw + aaddr + 32 * (d + 1) + 8 * u); });
                    const floatx4 bq = wl_ring[d];
#ifdef DMEL_ABLATE
                    if (p.flags & 0x800u) { acc0[0] += a_cur[0] + a_cur[1] + a_cur[2] + a_cur[3] + bq[0] + bq[1] + bq[2] + bq[3]; static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; a_cur[u] = a_nxt[u]; }); return; }   // timing only: no MFMAs
#endif
                    acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a_cur[0], bq[0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a_cur[1], bq[1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a_cur[2], bq[2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a_cur[3], bq[3], acc1, 0, 0, 0);
                    static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; a_cur[u] = a_nxt[u]; });
                };
                int s4 = 0;
                const int ring_n4 = DMEL_WL_UNCOND ? wl_last(n4, off4 - n4) : n4;
                for (; s4 + WL_DEPTH <= n4r; s4 += WL_DEPTH) {
                    static_for<0, WL_DEPTH>([&](auto dd) {
                        constexpr int d = decltype(dd)::value;
                        group(dd);
                        wl_bload(wl_ring[d], s4 + d + WL_DEPTH, ring_n4, off4 - n4);
                        if constexpr (DMEL_WL_UNCOND) {
                            // one group = the next group's A operands (two ds_read2), four MFMAs, the slot's refill -- in this order, group by group
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        }
                    });
                    aaddr += WL_DEPTH * 32;
                }
                static_for<0, WL_DEPTH - 1>([&](auto dd) { if (s4 + decltype(dd)::value < n4r) group(dd); });
                // the next phase's first groups: in flight under this phase's epilogue
                if (DMEL_WL_NEXT && ph + 1 < p.wl_phases) wl_ring_init(p.wl_len4[ph + 1], off4);
                floatx4 tot = acc0 + acc1;
                if constexpr (FPW == 1) {
                    // quads split over several blocks of this phase (the host's schedule, dmel_tables.cpp): the pieces' partial sums -- rows P
                    // and D of this wave's one frame -- are added across lanes, the piece that carries the mel band receives last
                    const int mg = p.wl_mg[ph];
                    if (mg != 0) {
                        // (the rows are copied out of the vector first: __builtin_bit_cast on the vector's ELEMENTS read element 0 both times --
                        // hipcc 7.2 emitted one ds_bpermute for the two -- and d lambd of g3_c3 came out wrong)
                        float r0 = tot[0], r1 = tot[1];
                        {
                            const int pa = (mi & 63) << 2;
                            const float t0 = __int_as_float(__builtin_amdgcn_ds_bpermute(pa, __float_as_int(r0)));
                            const float t1 = __int_as_float(__builtin_amdgcn_ds_bpermute(pa, __float_as_int(r1)));
                            if (mi & 0x10000) { r0 += t0; r1 += t1; }
                        }
                        if (mg & 2) {
                            const int pb = ((mi >> 8) & 63) << 2;
                            const float t0 = __int_as_float(__builtin_amdgcn_ds_bpermute(pb, __float_as_int(r0)));
                            const float t1 = __int_as_float(__builtin_amdgcn_ds_bpermute(pb, __float_as_int(r1)));
                            if (mi & 0x20000) { r0 += t0; r1 += t1; }
                        }
                        tot[0] = r0; tot[1] = r1;
                    }
                }
                // ---- epilogue: column j of block b = mel band li.y, rows = (frame, P | D) ----------------
                const int m = li.y;
                if (m < 0) continue;
#if DMEL_FWD_BAND
                if (!row_mine) continue;
#endif
#ifdef DMEL_ABLATE
                if (p.flags & 0x400u) { if (tot[0] == 12345.678f) out_clip[0] = tot[1] + tot[2] + tot[3]; continue; }   // timing only: no epilogue
                if (p.flags & 0x20000u) {
                    // timing only (values are wrong): the store pattern of a staged epilogue -- wave w writes rows 16 w .. 16 w + 15 of one
                    // tensor per phase, 64 contiguous bytes per row (this tile's 16 frames), 16 bytes per lane
                    const int mrow = 16 * wave + (lane >> 2);
                    float* q = (ph == 0 ? out_clip : (tan_clip ? tan_clip : out_clip)) + (unsigned)mrow * (unsigned)p.T + t0 + 4 * (lane & 3);
                    if (ph < 2 && mrow < p.M) *reinterpret_cast<float4*>(q) = make_float4(tot[0], tot[1], tot[2], tot[3]);
                    continue;
                }
#endif
                const unsigned rbase = (unsigned)m * (unsigned)p.T;
                float* orow = out_clip + rbase;
                unsigned short* orow_h = outh_clip + rbase;
                float* trow = tan_clip ? tan_clip + rbase : nullptr;
                float ov[FPW], tv[FPW];
                static_for<0, FPW>([&](auto ff) {
                    constexpr int f = decltype(ff)::value;
                    const float mel = 0.25f * tot[(FPW == 2) ? f : 0];
                    const float dmel = htan * tot[(FPW == 2) ? 2 + f : 1];
                    const float me = mel + p.eps;
                    ov[f] = do_log ? fast_log(me, p.eps) : mel;
                    tv[f] = do_log ? dmel * __builtin_amdgcn_rcpf(me) : dmel;
                });
                if (staged) {
                    static_for<0, NST>([&](auto pp) {
                        if (decltype(pp)::value == ph) {
                            sm[decltype(pp)::value] = m;
                            static_for<0, FPW>([&](auto ff) { constexpr int f = decltype(ff)::value; sv[decltype(pp)::value][f] = ov[f]; sv[decltype(pp)::value][FPW + f] = tv[f]; });
                        }
                    });
                    continue;
                }
                if constexpr (FPW == 2) {
                    if ((p.T & 1) == 0 && tA + 1 < p.T) {
                        // even T (tA is even): both frames of the wave as one aligned 8-byte store per tensor
                        if (out_bf16) *reinterpret_cast<unsigned*>(orow_h + tA) = (unsigned)bf16_bits(ov[0]) | ((unsigned)bf16_bits(ov[1]) << 16);
#ifdef DMEL_WL_NT
                        else __builtin_nontemporal_store(v2f{ov[0], ov[1]}, reinterpret_cast<v2f*>(orow + tA));
                        if (trow) __builtin_nontemporal_store(v2f{tv[0], tv[1]}, reinterpret_cast<v2f*>(trow + tA));
#else
                        else *reinterpret_cast<float2*>(orow + tA) = make_float2(ov[0], ov[1]);
                        if (trow) *reinterpret_cast<float2*>(trow + tA) = make_float2(tv[0], tv[1]);
#endif
                        continue;
                    }
                }
                static_for<0, FPW>([&](auto ff) {
                    constexpr int f = decltype(ff)::value;
                    const int t = tA + f;
                    if (t < p.T) {
                        if (out_bf16) orow_h[t] = bf16_bits(ov[f]); else orow[t] = ov[f];
                        if (trow) trow[t] = tv[f];
                    }
                });
            }
            STAMP(16 * ti + 9);   // contraction and epilogue arithmetic of all phases
            if (staged) {
                float* const stg = reinterpret_cast<float*>(smem_raw + wave * FPW * (SS * 8));          // [tensor][mel band][frame of this wave]
                static_for<0, NST>([&](auto pp) {
                    constexpr int q = decltype(pp)::value;
                    if (sm[q] >= 0) {
                        static_for<0, 2>([&](auto tt2) {
                            constexpr int pl = decltype(tt2)::value;
                            float* d = stg + ((pl * p.M + sm[q]) * FPW);
                            if constexpr (FPW == 2) *reinterpret_cast<float2*>(d) = make_float2(sv[q][pl * FPW], sv[q][pl * FPW + 1]);
                            else d[0] = sv[q][pl * FPW];
                        });
                    }
                });
                __syncthreads();
                STAMP(16 * ti + 10);
                constexpr int QPR = SLOTS / 4;                               // 16-byte pieces per row of the tile
#if DMEL_FWD_BAND
                const int srows = e_hi - e_lo, srow0 = e_lo;                 // only this channel's rows were staged
#else
                const int srows = p.M;
                constexpr int srow0 = 0;
#endif
                const int total = 2 * srows * QPR;
                // DMEL_WL_WT: the whole 16-byte pieces leave as write-through buffer stores (sc1) -- 1 = those of out, 2 = those of the
                // tangent, 3 = both, 0 = plain stores.  A plain store stays dirty in the XCD's L2 until the end-of-kernel release writes
                // 16 KB per workgroup back while nothing computes; a write-through one leaves while other workgroups still contract.
                // One descriptor per tensor and clip (in the band build: the shared image), M T 4 bytes; a clip image beyond what its
                // 32-bit range holds keeps the plain stores.  The shape guards below stay: a buffer store out of range is dropped silently.
#ifndef DMEL_WL_WT
#define DMEL_WL_WT 3
#endif
#if DMEL_WL_WT
                const unsigned long long img_bytes = (unsigned long long)p.M * (unsigned long long)p.T * 4ull;
                const bool wt_fits = img_bytes <= 0xffffffffull;
                const __amdgpu_buffer_rsrc_t r_out = make_rsrc(out_clip, wt_fits ? (unsigned)img_bytes : 0u);
                const __amdgpu_buffer_rsrc_t r_tan = make_rsrc(tan_clip, wt_fits ? (unsigned)img_bytes : 0u);
#endif
                for (int idx = tid; idx < total; idx += THREADS) {
                    const int rw = idx / QPR, c = idx % QPR;
                    const int pl = rw >= srows ? 1 : 0, mm = srow0 + rw - pl * srows;
                    float4 v;
                    if constexpr (FPW == 2) {
                        const float2 lo = *reinterpret_cast<const float2*>(smem_raw + (2 * c) * FPW * (SS * 8) + ((pl * p.M + mm) * FPW) * 4);
                        const float2 hi = *reinterpret_cast<const float2*>(smem_raw + (2 * c + 1) * FPW * (SS * 8) + ((pl * p.M + mm) * FPW) * 4);
                        v = make_float4(lo.x, lo.y, hi.x, hi.y);
                    } else {
                        float e[4];
                        static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; e[u] = *reinterpret_cast<const float*>(smem_raw + (4 * c + u) * (SS * 8) + (pl * p.M + mm) * 4); });
                        v = make_float4(e[0], e[1], e[2], e[3]);
                    }
                    float* dst = (pl ? tan_clip : out_clip) + (unsigned)mm * (unsigned)p.T + t0 + 4 * c;
                    const int t = t0 + 4 * c;
                    if (t + 3 < p.T) {
#if DMEL_WL_WT
                        // (a branch per tensor, not a descriptor chosen per lane: that would be a loop over the lanes' descriptors)
                        const unsigned eo = (unsigned)mm * (unsigned)p.T + t0 + 4 * c;   // element offset inside the clip's image
                        if ((DMEL_WL_WT & 1) && wt_fits && pl == 0) buf_store_wt_f4(r_out, eo * 4u, v);
                        else if ((DMEL_WL_WT & 2) && wt_fits && pl != 0) buf_store_wt_f4(r_tan, eo * 4u, v);
                        else
#endif
                        *reinterpret_cast<float4*>(dst) = v;
                    } else { if (t < p.T) dst[0] = v.x; if (t + 1 < p.T) dst[1] = v.y; if (t + 2 < p.T) dst[2] = v.z; }
                }
            }
            STAMP(16 * ti + 11);
        } else {
            // ================= phase 2: mel contraction on the matrix cores ======================
            const int row16 = lane & 15;
            const int slot8 = 2 * (row16 >> 2) + (row16 & 1);
            const int type = (row16 >> 1) & 1;
            const int kofs = lane >> 4;
            const int cg = lane >> 4;      // accumulator row group of this lane (C/D layout)
            const int col = lane & 15;

            const bool do_log = (p.flags & 1u) != 0;
            const bool out_bf16 = (p.flags & 4u) != 0;
            // ---- epilogue of one 16-mel tile: accumulators -> (B,1,M,T) -------------------------------
            auto write_tile = [&](int nt, const floatx4 (&tt)[MT]) {
                    if (nt < 0) return;
                    const int m = 16 * nt + col;
                    if (m >= p.M) return;
#if DMEL_FWD_BAND
                    if (m < e_lo || m >= e_hi) return;
#endif
                    const size_t rbase = ((size_t)FWD_BO * p.M + m) * p.T;
                    float* orow = p.out + rbase;
                    unsigned short* orow_h = reinterpret_cast<unsigned short*>(p.out) + rbase;     // DMEL_FLAG_OUT_BF16: out is bf16
                    float* trow = p.tangent ? p.tangent + rbase : nullptr;
                    auto put = [&](int t, float v) { if (out_bf16) orow_h[t] = bf16_bits(v); else orow[t] = v; };
                    static_for<0, MT>([&](auto mm) {
                        constexpr int mt = decltype(mm)::value;
                        const floatx4 a = tt[mt];
                        if constexpr (TRAINLIKE) {
                            // rows 4cg+i: i=0,1 -> |X|^2 of slots 2cg, 2cg+1; i=2,3 -> d|X|^2 of the same slots
                            const int tp = t0 + mt * 8 + 2 * cg;
                            if (((p.T | t0) & 1) == 0 && mt * 8 + 2 * cg + 1 < SLOTS && tp + 1 < p.T) {
                                // even T: both frames of this lane form one aligned 8-byte store per tensor
                                float2 o2, t2;
                                static_for<0, 2>([&](auto ss) {
                                    constexpr int s = decltype(ss)::value;
                                    const float mel = 0.25f * a[s];
                                    const float dmel = htan * a[2 + s];
                                    const float me = mel + p.eps;
                                    (s == 0 ? o2.x : o2.y) = do_log ? logf(me) : mel;
                                    (s == 0 ? t2.x : t2.y) = do_log ? dmel * __builtin_amdgcn_rcpf(me) : dmel;
                                });
                                if (out_bf16) *reinterpret_cast<unsigned*>(orow_h + tp) = (unsigned)bf16_bits(o2.x) | ((unsigned)bf16_bits(o2.y) << 16);
                                else *reinterpret_cast<float2*>(orow + tp) = o2;
                                if (trow) *reinterpret_cast<float2*>(trow + tp) = t2;
                            } else
                            static_for<0, 2>([&](auto ss) {
                                constexpr int s = decltype(ss)::value;
                                const int slot = mt * 8 + 2 * cg + s;
                                const int t = t0 + slot;
                                if (slot < SLOTS && t < p.T) {
                                    const float mel = 0.25f * a[s];
                                    const float dmel = htan * a[2 + s];
                                    if (do_log) {
                                        const float me = mel + p.eps;
                                        put(t, logf(me));
                                        if (trow) trow[t] = dmel * __builtin_amdgcn_rcpf(me);
                                    } else {
                                        put(t, mel);
                                        if (trow) trow[t] = dmel;
                                    }
                                }
                            });
                        } else {
                            // slot holds frames (2*slot, 2*slot+1) as (type 0, type 1)
                            static_for<0, 4>([&](auto ii) {
                                constexpr int i = decltype(ii)::value;
                                const int slot = mt * 8 + 2 * cg + (i & 1);
                                const int t = t0 + 2 * slot + (i >> 1);
                                if (slot < SLOTS && t < p.T) {
                                    const float mel = FWD_PAD_MEL(t, 0.25f * a[i]);
                                    put(t, do_log ? logf(mel + p.eps) : mel);
                                }
                            });
                        }
                    });
                };

            if constexpr (HSPLIT) {
                // ================= phase 2, dense bank on the bf16 matrix pipe ==============================
                // One v_mfma_f32_16x16x32_bf16 covers 32 bins: lane (row = lane & 15, kg = lane >> 4) supplies bins 32 ks + 8 kg .. + 7 of
                // its row's plane (one ds_read_b128 for hi, one for lo) and of its column of the filterbank (two 16-byte loads of the
                // pre-split table).  Three instructions of 16 cycles per (k-step, row tile) -- lo hi + hi lo + hi hi, smallest first --
                // against eight exact-fp32 ones of 32: the dense contraction's matrix time falls from ~14 us to ~2.5 us at BASELINE
                // config 2.  Wave w owns mel tile w of every group whole (a dense bank has no narrow and wide tiles to balance):
                // no half-tile exchange.  Bin N/2 -- N/2 bins are N/64 steps exactly -- rides on the vector pipe.
                typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
                constexpr int KS32 = N / 64;
                const int kgq = lane >> 4;
                int a_base[MT];
                static_for<0, MT>([&](auto mm) {
                    constexpr int mt = decltype(mm)::value;
                    const int slot = mt * 8 + slot8;
                    a_base[mt] = (slot < SLOTS ? slot : 0) * (SS * 8) + type * (2 * NHS * 2) + kgq * 16;
                });
                constexpr int TPWV = 8 / WAVES;                              // mel tiles of a group per wave (8 waves: 1, 4 waves: 2)
                for (int grp = 0; grp < p.groups; ++grp) {
                    static_for<0, TPWV>([&](auto jj) {
                        const int tile = grp * 8 + wave + WAVES * decltype(jj)::value;
                        if (16 * tile >= p.M) return;                       // (uniform per wave)
                        floatx4 acc[MT];
                        static_for<0, MT>([&](auto mm) { acc[decltype(mm)::value] = floatx4{0.f, 0.f, 0.f, 0.f}; });
                        const uint4* bt = p.ent_h + (size_t)tile * (KS32 * 2 * 64) + lane;
                        uint4 bh = bt[0], bl = bt[64];
                        for (int ks = 0; ks < KS32; ++ks) {
                            const uint4 ch = bh, cl = bl;
                            if (ks + 1 < KS32) { bh = bt[(ks + 1) * 128]; bl = bt[(ks + 1) * 128 + 64]; }
                            const bf16x8 vbh = __builtin_bit_cast(bf16x8, ch), vbl = __builtin_bit_cast(bf16x8, cl);
                            static_for<0, MT>([&](auto mm) {
                                constexpr int mt = decltype(mm)::value;
                                const bool valid = mt * 8 + slot8 < SLOTS;
                                uint4 ah = *reinterpret_cast<const uint4*>(smem_raw + a_base[mt] + ks * 64);
                                uint4 al = *reinterpret_cast<const uint4*>(smem_raw + a_base[mt] + NHS * 2 + ks * 64);
                                if constexpr (SLOTS < 8) { if (!valid) { ah = make_uint4(0, 0, 0, 0); al = ah; } }
                                const bf16x8 vah = __builtin_bit_cast(bf16x8, ah), val = __builtin_bit_cast(bf16x8, al);
                                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(val, vbh, acc[mt], 0, 0, 0);
                                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vah, vbl, acc[mt], 0, 0, 0);
                                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vah, vbh, acc[mt], 0, 0, 0);
                            });
                        }
                        // bin N/2: rows 4 cg + i of the accumulator layout -> (slot 2 cg + (i & 1), P | D = i >> 1)
                        const int mcol = 16 * tile + col;
                        const float fbn = mcol < p.M ? p.fb_nyq[mcol] : 0.f;
                        static_for<0, MT>([&](auto mm) {
                            constexpr int mt = decltype(mm)::value;
                            static_for<0, 4>([&](auto ii) {
                                constexpr int i = decltype(ii)::value;
                                const int slot = mt * 8 + 2 * cg + (i & 1);
                                if (slot < SLOTS) acc[mt][i] = fmaf(load_h(slot * (SS * 8), i >> 1, N / 2), fbn, acc[mt][i]);
                            });
                        });
                        write_tile(tile, acc);
                    });
                }
            } else
            for (int grp = 0; grp < p.groups; ++grp) {
                // acc[loc][mt][parity]: two accumulators per tile so that consecutive MFMAs never wait on each other
                floatx4 acc[NLOC][MT][2];
                static_for<0, NLOC>([&](auto l) { static_for<0, MT>([&](auto m) { static_for<0, 2>([&](auto e) {
                    acc[decltype(l)::value][decltype(m)::value][decltype(e)::value] = floatx4{0.f, 0.f, 0.f, 0.f}; }); }); });
                int tile_of[NLOC];
                int helpers = 0;         // bit w set = wave w's run 1 is a piece of THIS wave's tile (bits 16-23 of run 0's tile word)
                bool piece1 = (WAVES == 8);   // run 1 is a piece of another wave's tile (always with 8 waves; bit 30 of its tile word with 4)
                static_for<0, NLOC>([&](auto l) {
                    constexpr int loc = decltype(l)::value;
                    // (ks0, nks, boff, tile): the filterbank is banded, so the non-zero 4x16 blocks of one mel tile
                    // form ONE contiguous run of k-steps; nks is padded to a multiple of 4 with zero blocks
                    int4 tr = tr0[loc];
                    if (grp > 0) tr = p.tile_ranges[(grp * WAVES + wave) * NLOC + loc];
                    const int ks0 = __builtin_amdgcn_readfirstlane(tr.x), nks = __builtin_amdgcn_readfirstlane(tr.y);
                    const int boff = __builtin_amdgcn_readfirstlane(tr.z);
                    {
                        const int tw = __builtin_amdgcn_readfirstlane(tr.w);
                        tile_of[loc] = tw < 0 ? -1 : (tw & 0xffff);
                        if constexpr (loc == 0) helpers = tw < 0 ? 0 : ((tw >> 16) & 0xff);
                        if constexpr (loc == 1 && WAVES != 8) piece1 = tw >= 0 && ((tw >> 30) & 1) != 0;
                    }
#ifdef DMEL_ABLATE
                    if (p.flags & 0x800u) return;                       // timing ablation: skip the MFMA loop
#endif
                    if (nks <= 0) return;
#if DMEL_FWD_BAND
                    // a mel tile (or a piece of one) none of whose 16 bands is this channel's: nothing of it is stored, so nothing is contracted
                    // (uniform: the tile word is in scalar registers; the exchange below still runs, on zeros)
                    if (DMEL_BAND_SKIP && tile_of[loc] >= 0 && (16 * tile_of[loc] + 16 <= e_lo || 16 * tile_of[loc] >= e_hi)) return;
#endif
                    const int bbase = (boff + lane) * 4;
                    // One group = 4 consecutive k-steps = 16 consecutive bins starting at a multiple of 16 (the host
                    // aligns every run to 4 k-steps), so the 4 reads of Z[k] share one base address and, except at one
                    // bin per 256, so do the 4 reads of the mirrored Z[N-k].
                    // A operands of one group: 4 LDS reads per 16-row tile
                    auto load_a = [&](int ksg, float (&av)[MT][4]) {
                        const int k0 = 4 * ksg + kofs;                               // bin of k-step 0 for this lane
                        const int zk0 = z_index<R, C>(k0 & (N - 1));
                        static_for<0, MT>([&](auto m) {
                            constexpr int mt = decltype(m)::value;
                            const int slot = mt * 8 + slot8;
                            const bool valid = slot < SLOTS;
                            // rows of type 0 read PD.x (|S|^2), rows of type 1 PD.y: the A operand is a plain 4-byte LDS read
                            const float* slf = reinterpret_cast<const float*>(lds + (valid ? slot : 0) * SS) + type;
                            static_for<0, 4>([&](auto uu) { constexpr int u = decltype(uu)::value; av[mt][u] = slf[2 * (zk0 + 4 * u)]; });
                        });
                    };
                    auto mfma4 = [&](const float (&av)[MT][4], float b0, float b1, float b2, float b3) {
                        const float bq[4] = {b0, b1, b2, b3};
                        static_for<0, MT>([&](auto m) {
                            constexpr int mt = decltype(m)::value;
                            const bool valid = mt * 8 + slot8 < SLOTS;
                            static_for<0, 4>([&](auto uu) {
                                constexpr int u = decltype(uu)::value;
                                float val = av[mt][u];
                                if constexpr (SLOTS < 8) val = valid ? val : 0.f;
                                acc[loc][mt][u & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(val, bq[u], acc[loc][mt][u & 1], 0, 0, 0);
                            });
                        });
                    };
                    // With two waves per SIMD (n_fft >= 4096) nobody covers the LDS round trip between the reads of a group and its
                    // MFMAs: a wave with a long run spent ~85 cycles per MFMA instead of 32.  There the A operands of the NEXT group are
                    // requested before the MFMAs of this one (reads past the run land on valid bins and are not used).  With four
                    // waves per SIMD the same prefetch measured slower (23.5 against 23.4 us at config 2) and is not compiled in.
                    constexpr bool APRE = (N >= 4096);       // ESC-50 shape: 157.5 -> 154.5 us at n_fft 4096, 486 -> 476 at 8192
                    float a_cur[MT][4];
                    if constexpr (APRE) load_a(ks0, a_cur);
                    auto group4 = [&](int ksg, float b0, float b1, float b2, float b3) {
                        if constexpr (APRE) {
                            float a_nxt[MT][4];
                            load_a(ksg + 4, a_nxt);
                            mfma4(a_cur, b0, b1, b2, b3);
                            static_for<0, MT>([&](auto m) { static_for<0, 4>([&](auto uu) { a_cur[decltype(m)::value][decltype(uu)::value] = a_nxt[decltype(m)::value][decltype(uu)::value]; }); });
                        } else {
                            float av[MT][4];
                            load_a(ksg, av);
                            mfma4(av, b0, b1, b2, b3);
                        }
                    };
                    if (grp == 0) {
                        // k-steps whose B fragments are already in registers
                        static_for<0, NBPRE / 4>([&](auto qq) {
                            constexpr int i = decltype(qq)::value * 4;
                            // (running the padding groups too, branch-free on zero fragments, was measured: 24.6 against 21.9 us at
                            // config 2 -- the matrix pipe of a SIMD serialises the four waves that reach this phase together)
                            if (i < nks) group4(ks0 + i, bpre[loc][i], bpre[loc][i + 1], bpre[loc][i + 2], bpre[loc][i + 3]);
                        });
                    }
                    // the rest (long runs: dense custom filterbanks, further mel groups) streams with a 4-step prefetch
                    const int istart = (grp == 0) ? NBPRE : 0;
                    if (istart < nks) {
                        // a ring of DEPTH groups of 4 fragments in flight: one group ahead left the loop waiting for an L2 round trip per
                        // 4 MFMAs (dense banks -- a trainable filterbank -- and the long runs of n_fft >= 4096 live in this loop);
                        // offsets past the run are range-checked by the buffer descriptor or read the next run: never used
                        // (4 deep: n_fft 4096 at the reference's ESC-50 shape 171 -> 163 us, 8192 530 -> 512; at 2048 the 8 extra
                        // registers spill and config 3 went 49.8 -> 51.9 us, so the sizes with 128 VGPRs keep two groups)
                        constexpr int DEPTH = (N >= 4096) ? 4 : 2;
                        float br[DEPTH][4];
                        static_for<0, DEPTH>([&](auto dd) {
                            constexpr int d = decltype(dd)::value;
                            static_for<0, 4>([&](auto u) { br[d][decltype(u)::value] = buf_f32(rb, bbase + (istart + 4 * d + decltype(u)::value) * 256); });
                        });
                        for (int i = istart; i < nks; i += 4 * DEPTH) {
                            static_for<0, DEPTH>([&](auto dd) {
                                constexpr int d = decltype(dd)::value;
                                if (i + 4 * d < nks) {
                                    group4(ks0 + i + 4 * d, br[d][0], br[d][1], br[d][2], br[d][3]);
                                    static_for<0, 4>([&](auto u) { br[d][decltype(u)::value] = buf_f32(rb, bbase + (i + 4 * (d + DEPTH) + decltype(u)::value) * 256); });
                                }
                            });
                        }
                    }
                });
                STAMP(16 * ti + 9);   // MFMA loops
                // ---- epilogue: accumulators -> (B,1,M,T) ------------------------------------------
                floatx4 tot[NLOC][MT];
                static_for<0, NLOC>([&](auto l) { static_for<0, MT>([&](auto m) {
                    tot[decltype(l)::value][decltype(m)::value] = acc[decltype(l)::value][decltype(m)::value][0] + acc[decltype(l)::value][decltype(m)::value][1]; }); });
                if (WAVES == 8 || ((p.xch_groups >> (grp & 31)) & 1u)) {
                    // run 1 of a wave is a piece of some OTHER wave's tile (the host deals the k-steps of the wide tiles over the
                    // waves with narrow or no tiles of their own: build_b_stream, dmel_tables.cpp): every wave leaves its run-1 sums in its own slot
                    // and an owner adds the slots of its helpers in ascending order (fixed order: deterministic)
                    // (one 16-row tile at a time through the same 8 KB: two tiles at once would put the 16-frame workgroup of
                    // n_fft 1024 past half of the CU's LDS)
                    floatx4* xch = reinterpret_cast<floatx4*>(smem_raw + SLOTS * SS * 8);
                    static_for<0, MT>([&](auto mm) {
                        constexpr int mt = decltype(mm)::value;
                        if constexpr (mt > 0) __syncthreads();
                        xch[wave * 64 + lane] = piece1 ? tot[1][mt] : floatx4{0.f, 0.f, 0.f, 0.f};
                        __syncthreads();
                        static_for<0, WAVES>([&](auto ss) {
                            constexpr int sw = decltype(ss)::value;
                            if (helpers & (1 << sw)) tot[0][mt] += xch[sw * 64 + lane];
                        });
                    });
                    if (p.groups > 1) __syncthreads();
                    if (piece1) tile_of[1] = -1;
                }
                STAMP(16 * ti + 10);  // half-tile exchange
#ifdef DMEL_ABLATE
                if (p.flags & 0x400u) continue;                        // timing ablation: skip the epilogue
#endif
                static_for<0, NLOC>([&](auto l) { write_tile(tile_of[decltype(l)::value], tot[decltype(l)::value]); });
                STAMP(16 * ti + 11);  // epilogue stores issued
            }
        }
    });
}

#undef FWD_BO
#undef FWD_LAM
#undef FWD_WIN2
#undef FWD_LEADER
#undef FWD_KERNEL
#undef FWD_PARAMS
#undef FWD_LC
#undef FWD_INV_L
#undef FWD_TC
#undef FWD_PAD_MEL
#undef FWD_LIM_A
#undef FWD_LIM_B
#undef FWD_FILL_ROWS
#undef FWD_FILL_ROW
