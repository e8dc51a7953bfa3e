// dmel_xgrad_wave_body.inc -- the wave-FFT kernel of the gradient w.r.t. the waveform.  Six builds, chosen by the macros set at the #include:
//
//   DMEL_XG_MULTI  DMEL_XG_BAND  DMEL_XG_LEN   kernel                              parameters            file
//   0              -             -             dmel_xgrad_wave_kernel              XgradParams           dmel_xgrad.hip
//   1              -             -             dmel_xgrad_wave_multi_kernel        XgradMultiParams      dmel_xgrad.hip
//   0              -             1             dmel_xgrad_wave_len_kernel          XgradLenParams        dmel_xgrad_len.hip
//   1              1             -             dmel_xgrad_wave_band_kernel         XgradBandParams       dmel_xgrad_band.hip
//   1              -             1             dmel_xgrad_wave_multi_len_kernel    XgradMultiLenParams   dmel_xgrad_klen.hip
//   1              1             1             dmel_xgrad_wave_band_len_kernel     XgradBandLenParams    dmel_xgrad_klen.hip
//
// MULTI: the channel slot comes out of the relabelled workgroup index, as in dmel_fwd_multi_kernel.  BAND: the multi kernel's channel slot with
// ONE image behind grad_out / out; a channel stages only its own rows of it, every other row of gm is +0.0.  LEN: clips of per-clip lengths.
// The XG_* names below expand, for the two kernels of dmel_xgrad.hip, to exactly the tokens they were written with.
#if DMEL_XG_BAND && DMEL_XG_LEN
#define XG_KERNEL dmel_xgrad_wave_band_len_kernel
#define XG_PARAMS XgradBandLenParams mp
#define XG_BO b
#elif DMEL_XG_BAND
#define XG_KERNEL dmel_xgrad_wave_band_kernel
#define XG_PARAMS XgradBandParams mp
#define XG_BO b
#elif DMEL_XG_MULTI && DMEL_XG_LEN
#define XG_KERNEL dmel_xgrad_wave_multi_len_kernel
#define XG_PARAMS XgradMultiLenParams mp
#define XG_BO bo
#elif DMEL_XG_MULTI
#define XG_KERNEL dmel_xgrad_wave_multi_kernel
#define XG_PARAMS XgradMultiParams mp
#define XG_BO bo
#elif DMEL_XG_LEN
#define XG_KERNEL dmel_xgrad_wave_len_kernel
#define XG_PARAMS XgradLenParams p
#define XG_BO b
#else
#define XG_KERNEL dmel_xgrad_wave_kernel
#define XG_PARAMS XgradParams p
#define XG_BO b
#endif
// sample-space bounds of a clip: L (also the row stride of x) and fl32(1 / L), or the clip's own length Lc (dmel_xgrad_wave_len_kernel); its
// frames: T (also the row stride of grad_out / out), or Tc
#if DMEL_XG_LEN
#if DMEL_XG_MULTI
#define XG_LENGTHS mp.lengths
#else
#define XG_LENGTHS p.lengths
#endif
#define XG_LC Lc
#define XG_PSUM_L Lc
#define XG_INV_L inv_Lc
#define XG_TC Tc
#else
#define XG_LC L
#define XG_PSUM_L p.L
#define XG_INV_L p.inv_L
#define XG_TC T
#endif
// the indices of gm (M, FPT) that are staged from memory end here: all of it, or the channel's rows [e_lo, e_hi) (dmel_xgrad_wave_band_kernel)
// (and the element a masked-off request reads instead: one of the channel's own)
#if DMEL_XG_BAND
#define XG_GM_END g_end
#define XG_GM_SAFE (unsigned)(e_lo * T)
#else
#define XG_GM_END total
#define XG_GM_SAFE 0u
#endif
template <int N>
__global__ void __launch_bounds__((XgPlan<N>::THREADS), (XgPlan<N>::MINW)) XG_KERNEL(XG_PARAMS)
{
#if DMEL_XG_MULTI
    XgradParams p = mp.p;                                         // its per-channel fields are set below
#endif
    using PL = XgPlan<N>;
    constexpr int R = PL::R, C = PL::C, G = PL::G, FPW = PL::FPW, SLOTS = PL::SLOTS, FPT = PL::FPT;
    constexpr int THREADS = PL::THREADS, SS = PL::SS, RR = R * R;
    constexpr int NPAIR = N / (2 * G) + 1;                       // bins lg + G i <= N/2
    constexpr int PADC = (C > 1) ? 4 : 0;                         // spectrum index k + PADC (k / R^2), as the forward (z_index)
    constexpr int PADP = PL::PADP;                                // frame-gradient planes: n + PADP (n / R^2)
    static_assert(G <= 64 && N == R * R * C && RR % G == 0, "one wave (or a part of it) per frame pair");
    static_assert(N + (C - 1) * PADP <= SS, "a plane of frame gradients fits half a slot");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
#if !DMEL_XG_MULTI
    if (xgrad_not_this_nfft(p)) return;
#endif
    v2f* lds = reinterpret_cast<v2f*>(smem_raw);
    float* win = reinterpret_cast<float*>(smem_raw + SLOTS * SS * 8);
    // the window table: entries 0 .. N/2 when it is symmetric about N/2 (the Gaussian of the optimized=True branch), else all N
    const int WN = p.win_n;
    const bool sym = WN < N;
    float* gm = win + ((WN + 3) & ~3);                            // (M, FPT); later the fp64 partial sums
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int wg = blockIdx.x;
    {   // contiguous tiles per XCD (neighbouring tiles share samples: L2 hits), as the forward
        const int nwg = gridDim.x, q = nwg >> 3, rr = nwg & 7, xcd = wg & 7;
        wg = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (wg >> 3);
    }
#if DMEL_XG_MULTI
    // multi-window layer: the channel slot comes out of the relabelled index, so that a channel's tiles keep the placement above.  The
    // channel's lambd (device word or host value), window table, segment and csum regions replace the launch's; with lambd on the device a
    // workgroup returns at once unless lambd[ch] asks for THIS n_fft (DMEL_FLAG_CHECK_NFFT per channel)
    const int cslot = wg / mp.ch_grid;
    wg -= cslot * mp.ch_grid;
    const int ch = (int)((mp.ch_list >> (4 * cslot)) & 15u);
    if (p.lam_dev) p.lam_dev += ch;
    p.win_denom = mp.win_denom[ch];
    p.win2 = mp.win2[ch];
    p.frames = mp.frames[ch];
    p.csum = mp.csum[ch];
    p.spec_mode = 0;
    if (xgrad_not_this_nfft(p)) return;
#endif
    XSTAMP(0);
    const int tiles = p.tiles, M = p.M, T = p.T, hop = p.hop, L = p.L;
    const int b = wg / tiles, tile = wg % tiles;
#if DMEL_XG_LEN
    // the clip is x[b, :Lc] (one scalar load: uniform over the workgroup) with Tc = Lc / hop + 1 frames; the frames past them are pad frames
    // (zero mel gradient).  A tile whose first frame is a pad frame, and every tile of a clip whose length is outside 1 ... L, does nothing:
    // dmel_xgrad_combine_len_kernel (dmel_xgrad_combine_multi_len_kernel) reads neither its segment nor its sum.
    const ClipLen cl = clip_len(XG_LENGTHS, b, L, hop);
    const int Lc = cl.Lc, Tc = cl.Tc;
    const float inv_Lc = 1.0f / (float)Lc;
    if (!cl.ok || tile * FPT >= Tc) return;
#endif
#if DMEL_XG_MULTI && !DMEL_XG_BAND
    const int bo = b * mp.ch_out + ch;                            // the clip's row of grad_out / out: (B, K, M, T)
#endif
    const int t0 = tile * FPT;
    const int j = lane / G, lg = lane % G;
    const int slot = wave * FPW + j;
    v2f* sl = lds + slot * SS;
    const int slot_b = slot * (SS * 8);
    const int tA = t0 + 2 * slot;
    const int f0 = tA * hop - N / 2;                              // first sample of frame tA; frame tA + 1 starts hop later
    // samples of both frames: plain offsets when the pair lies inside the clip, else clamped (and zeroed at windowing time)
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x + (size_t)b * L, (unsigned)XG_LC * 4u);
    const bool inside = __all((f0 >= 0) && (f0 + hop + N <= XG_LC));
    float xa[R], xc[R];
    if (inside) {
        static_for<0, R>([&](auto aa) {
            constexpr int a = decltype(aa)::value;
            xa[a] = buf_f32(rx, (f0 + lg + G * a) * 4);
            xc[a] = buf_f32(rx, (f0 + hop + lg + G * a) * 4);
        });
    } else {
        static_for<0, R>([&](auto aa) {
            constexpr int a = decltype(aa)::value;
            xa[a] = buf_f32(rx, clampi(f0 + lg + G * a, XG_LC - 1) * 4);
            xc[a] = buf_f32(rx, clampi(f0 + hop + lg + G * a, XG_LC - 1) * 4);
        });
    }
    // everything else the prologue needs is requested before anything is waited for: the first batch of gm (four words per
    // thread: the whole tile at BASELINE config 2), the window entries, the clip's partial sums
    const int total = p.spec_mode ? 0 : M * FPT;
    const float* gb = p.grad_out + (size_t)XG_BO * M * T;
    const float* yb = p.out ? p.out + (size_t)XG_BO * M * T : nullptr;
    // (requests only: nothing here touches what was loaded -- a select on a loaded value, or a branch around a load, makes the
    // compiler wait for it on the spot, and vector loads return in order: that wait would also sit out the 2 R sample loads above)
    const float* ysrc = yb ? yb : gb;                                             // always a valid address; ignored without the log
#if DMEL_XG_BAND
    // the channel's rows of the image (uniform: scalar registers, as dmel_fwd_band_kernel): indices g_lo ... g_end - 1 of gm come from
    // memory, in as many round trips as the group's share of the rows needs; the other rows are never requested -- in log mode they hold
    // other channels' output, which must not reach exp(-y) -- and are written as +0.0 below
    const int e_lo = __builtin_amdgcn_readfirstlane(mp.band_edges[ch]), e_hi = __builtin_amdgcn_readfirstlane(mp.band_edges[ch + 1]);
    const int g_lo = e_lo * FPT, g_end = e_hi * FPT;
#endif
    auto gm_fetch = [&](int base, float (&v)[4], float (&y)[4]) {
        static_for<0, 4>([&](auto uu) {
            constexpr int u = decltype(uu)::value;
            const int idx = base + u * THREADS, m = idx / FPT, t = t0 + idx % FPT;
            const bool ok = idx < XG_GM_END && t < XG_TC;
            const unsigned o = ok ? (unsigned)(m * T + t) : XG_GM_SAFE;
            v[u] = gb[o];
            y[u] = ysrc[o];
        });
    };
    auto gm_store = [&](int base, const float (&v)[4], const float (&y)[4]) {
        static_for<0, 4>([&](auto uu) {
            constexpr int u = decltype(uu)::value;
            const int idx = base + u * THREADS, t = t0 + idx % FPT;
            if (idx < XG_GM_END) {
                const float val = yb ? v[u] * expf(-y[u]) : v[u];
                gm[idx] = t < XG_TC ? val : 0.f;
            }
        });
    };
    float gv[4], gy[4];
#if DMEL_XG_BAND
    gm_fetch(g_lo + tid, gv, gy);
#else
    if (total > 0) gm_fetch(tid, gv, gy);
#endif
    constexpr int WPT = (N + THREADS - 1) / THREADS;
    float mean = 0.f;
    if (p.own_prep) {
        // short clips, plain Gaussian window: no dmel_prep_kernel launch.  The window (time_frequency.py:21-30, the fp32 expression of
        // the forward) is evaluated here, and every workgroup adds up its clip itself in a fixed order (models.py:38; L2 hits
        // after the first toucher): requests in batches of 8 per thread, one round trip per batch.
        const float* xc = p.x + (size_t)b * L;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int i0 = 0;
        constexpr int KB = 8;
        if ((reinterpret_cast<uintptr_t>(xc) & 15) == 0) {
            const float4* x4 = reinterpret_cast<const float4*>(xc);
            const int n4 = XG_LC / 4;
            for (int base = 0; base < n4; base += THREADS * KB) {
                float4 v[KB];
                static_for<0, KB>([&](auto jj) {
                    constexpr int jv = decltype(jj)::value;
                    const int q = base + tid + THREADS * jv;
                    v[jv] = x4[q < n4 ? q : n4 - 1];
                });
                static_for<0, KB>([&](auto jj) {
                    constexpr int jv = decltype(jj)::value;
                    const bool ok = base + tid + THREADS * jv < n4;
                    a0 += ok ? v[jv].x : 0.f; a1 += ok ? v[jv].y : 0.f; a2 += ok ? v[jv].z : 0.f; a3 += ok ? v[jv].w : 0.f;
                });
            }
            i0 = n4 * 4;
        }
        for (int i = i0 + tid; i < XG_LC; i += THREADS) a0 += xc[i];
        // lambd by value, or read here from the parameter's storage (a uniform scalar load; dmel_backward_x_dev: no host read)
        float win_denom = p.win_denom;
        if (p.lam_dev) win_denom = __builtin_fabsf(*(const __attribute__((address_space(4))) float*)p.lam_dev) + 1e-15f;   // scalar load: see lam_load
        static_for<0, WPT>([&](auto ww) {
            constexpr int wi = decltype(ww)::value;
            const int n = tid + THREADS * wi;
            if (n < WN) {
                const float d = (float)n - (float)N / 2.0f;
                const float tq = d / win_denom;
                win[n] = expf(-0.5f * (tq * tq));
            }
        });
        // the forward's mean (dmel_kernels.h: "the clip mean"): fp32 tree, quotient rounded once
        float ps = wave_sum((a0 + a1) + (a2 + a3));
        float* redm = reinterpret_cast<float*>(smem_raw + p.tw2_off + (C > 1 ? R * C * 8 : 0));
        if (lane == 0) redm[wave] = ps;
        __syncthreads();
        float tot = 0.f;
        for (int q = 0; q < THREADS / 64; ++q) tot += redm[q];
        mean = mean_quotient(tot, XG_LC, XG_INV_L);
    } else {
        float wv[WPT];
        static_for<0, WPT>([&](auto ww) { constexpr int wi = decltype(ww)::value; const int n = tid + THREADS * wi; wv[wi] = p.win2[n < WN ? n : 0].x; });
        mean = clip_mean_psum(p.psum, p.nchunks, b, XG_PSUM_L);
        static_for<0, WPT>([&](auto ww) { constexpr int wi = decltype(ww)::value; const int n = tid + THREADS * wi; if (n < WN) win[n] = wv[wi]; });
    }
#if DMEL_XG_BAND
    {
        gm_store(g_lo + tid, gv, gy);
        for (int base = g_lo + tid + 4 * THREADS; base < g_end; base += 4 * THREADS) { gm_fetch(base, gv, gy); gm_store(base, gv, gy); }
        // the rows of the other channels, and row M (zeros, read as "the next row" of row M - 1): +0.0, what the scalar kernel forms
        // from a cotangent whose rows outside [e_lo, e_hi) are +0.0
        for (int i = tid; i < g_lo; i += THREADS) gm[i] = 0.f;
        for (int i = g_end + tid; i < total + FPT; i += THREADS) gm[i] = 0.f;
    }
#else
    if (total > 0) {
        gm_store(tid, gv, gy);
        for (int base = tid + 4 * THREADS; base < total; base += 4 * THREADS) { gm_fetch(base, gv, gy); gm_store(base, gv, gy); }
        if (tid < FPT) gm[total + tid] = 0.f;                                     // row M: zeros, read as "the next row" of row M - 1
    }
#endif
    // the radix-C twiddles through LDS (R x C entries: a wave-wide global load of them would still move 512 B per p1)
    float2* tw2l = reinterpret_cast<float2*>(smem_raw + p.tw2_off);
    if (C > 1 && tid < R * C) tw2l[tid] = p.tw2[tid];
    XSTAMP(1);   // prologue issued
    __syncthreads();
    XSTAMP(2);   // ... and complete

    // ---- forward transform of the pair: Z = FFT(x~_a w + i x~_b w)
    {
        v2f z[R];
        // window entries n = lg + G a: the first half directly, the second half mirrored when only half the table is kept
        const int wlo = lg, whi = sym ? N - lg : lg;
        const int whs = sym ? -G : G;
        static_for<0, R>([&](auto aa) {
            constexpr int a = decltype(aa)::value;
            const float w = (a < R / 2) ? win[wlo + G * a] : win[whi + whs * a];
            if (inside) z[a] = v2f{xa[a] - mean, xc[a] - mean} * splat(w);
            else {
                const int ia = f0 + lg + G * a, ib = ia + hop;
                const float va = (ia >= 0 && ia < XG_LC) ? xa[a] - mean : 0.f;
                const float vb = (ib >= 0 && ib < XG_LC) ? xc[a] - mean : 0.f;
                z[a] = v2f{va, vb} * splat(w);
            }
        });
        wave_fft<R, C, G>(z, sl, lg, p.tw1, tw2l, [&](auto pp1, int qp, int p2, v2f v) {
            constexpr int p1 = decltype(pp1)::value;
            sl[qp + (RR + PADC) * p2 + R * p1] = v;
        });
    }
    wave_sync();
    XSTAMP(3);   // first transform
    // ---- bin by bin: the two spectra, the gradient of the power spectrum, conj(H_a + i H_b) back in place.
    // Addresses as in the forward's pairing pass: a per-lane byte base plus a compile-time offset --
    //   Z[k],   k = lg + G i:   zb + 8 (G i + pad(G i))
    //   Z[N-k], lg >= 1:        mb + 8 (c_i + pad(c_i)),  mb = slot + 8 (G - lg),  c_i = N - G (i + 1)
    //   lane 0: N - G i itself; one padding step further when it starts an R*R block (mbA), bin 0 for i = 0 (mb0)
    {
        v2f wk[NPAIR], wn[NPAIR];
        const bool hasA = tA < XG_TC, hasB = tA + 1 < XG_TC;
        // row k of the filterbank as (c0, c1, first column, columns): an HTK row has two non-zero columns, and consecutive lanes
        // read consecutive 16-byte entries (the coefficients themselves lie a whole row of M floats apart: 64 cache lines per
        // load).  Rows with more columns (a trained, dense bank: p.long_rows, uniform) add the rest from the matrix.
        float4 rk[NPAIR];
        if (!p.spec_mode) {
            static_for<0, NPAIR>([&](auto ii) {
                constexpr int i = decltype(ii)::value;
                rk[i] = p.rowpk[(i < NPAIR - 1 || lg == 0) ? lg + G * i : 0];
            });
        }
        int zb = slot_b + lg * 8;
        int mb = slot_b + (G - lg) * 8;
        int mbA = mb + ((lg == 0) ? PADC * 8 : 0);
        int mb0 = (lg == 0) ? slot_b : mb + (N - G + PADC * ((N - G) / RR)) * 8;       // full address of Z[N-k] for i = 0
        asm volatile("" : "+v"(zb), "+v"(mb), "+v"(mbA), "+v"(mb0));
        const float* gcol0 = gm + 2 * slot;                                           // this pair's two columns of gm
        static_for<0, NPAIR>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            constexpr int ck = G * i, cm = N - G * (i + 1);
            constexpr bool crossing = PADC != 0 && ((N - G * i) % RR) == 0;
            const int mbase = (i == 0) ? mb0 : (crossing ? mbA : mb);
            const v2f zk = *reinterpret_cast<const v2f*>(smem_raw + zb + (ck + PADC * (ck / RR)) * 8);
            const v2f zn = *reinterpret_cast<const v2f*>(smem_raw + mbase + ((i == 0) ? 0 : (cm + PADC * (cm / RR)) * 8));
            // X_a = (Z_k + conj Z_{N-k}) / 2,  X_b = (Z_k - conj Z_{N-k}) / (2i)
            const float xar = 0.5f * (zk.x + zn.x), xai = 0.5f * (zk.y - zn.y);
            const float xbr = 0.5f * (zk.y + zn.y), xbi = -0.5f * (zk.x - zn.x);
            float gpa = 0.f, gpb = 0.f;
            if (p.spec_mode) {
                const int kc = (i < NPAIR - 1 || lg == 0) ? lg + G * i : 0;
                const float* gs = p.grad_out + ((size_t)b * p.F + kc) * T + tA;
                gpa = hasA ? gs[0] : 0.f;
                gpb = hasB ? gs[1] : 0.f;
            } else {
                const int b0 = __builtin_bit_cast(int, rk[i].z);
                const float* gcol = gcol0 + b0 * FPT;
                const float2 ga = *reinterpret_cast<const float2*>(gcol);
                const float2 gb2 = *reinterpret_cast<const float2*>(gcol + FPT);      // (row M of gm exists and is zero)
                gpa = fmaf(rk[i].y, gb2.x, rk[i].x * ga.x);
                gpb = fmaf(rk[i].y, gb2.y, rk[i].x * ga.y);
                if (p.long_rows) {
                    const int nb = __builtin_bit_cast(int, rk[i].w);
                    const float* fr = p.fb + (size_t)((i < NPAIR - 1 || lg == 0) ? lg + G * i : 0) * M;
                    for (int m = b0 + 2; m < b0 + nb; ++m) {
                        const float c = fr[m];
                        const float2 g2 = *reinterpret_cast<const float2*>(gcol0 + m * FPT);
                        gpa = fmaf(c, g2.x, gpa);
                        gpb = fmaf(c, g2.y, gpb);
                    }
                }
            }
            // k = 0 and k = N/2 (lane 0 of the first / last round): X is real there and the bin is its own mirror image
            if constexpr (i == 0 || i == NPAIR - 1) {
                const bool edge = (lg == 0);
                const float sc = edge ? 2.f : 1.f;
                const float har = sc * gpa * xar, hai = edge ? 0.f : gpa * xai;
                const float hbr = sc * gpb * xbr, hbi = edge ? 0.f : gpb * xbi;
                wk[i] = v2f{har - hbi, -(hai + hbr)};
                wn[i] = v2f{har + hbi, hai - hbr};
            } else {
                const float har = gpa * xar, hai = gpa * xai, hbr = gpb * xbr, hbi = gpb * xbi;
                wk[i] = v2f{har - hbi, -(hai + hbr)};                             // conj(H_a + i H_b) at k
                wn[i] = v2f{har + hbi, hai - hbr};                                // ... at N - k (Hermitian extension)
            }
        });
        wave_sync();                                                              // every read of Z precedes the first write
        static_for<0, NPAIR>([&](auto ii) {
            constexpr int i = decltype(ii)::value;
            constexpr int ck = G * i, cm = N - G * (i + 1);
            constexpr bool crossing = PADC != 0 && ((N - G * i) % RR) == 0;
            const int mbase = (i == 0) ? mb0 : (crossing ? mbA : mb);
            const bool edge = (lg == 0) && (i == 0 || i == NPAIR - 1);
            if (i < NPAIR - 1 || lg == 0) {                                       // the last round holds only the Nyquist bin
                *reinterpret_cast<v2f*>(smem_raw + zb + (ck + PADC * (ck / RR)) * 8) = wk[i];
                if (!edge) *reinterpret_cast<v2f*>(smem_raw + mbase + ((i == 0) ? 0 : (cm + PADC * (cm / RR)) * 8)) = wn[i];
            }
        });
    }
    wave_sync();
    XSTAMP(4);   // bin pass
    // ---- second transform: FFT(conj U) = conj(dv_a + i dv_b); windowed, the two frame gradients go to the two halves of the slot
    // (one plane of N floats each: the overlap-add below then reads consecutive words)
    float* pl = reinterpret_cast<float*>(sl);
    {
        v2f z[R];
        static_for<0, R>([&](auto aa) {
            constexpr int a = decltype(aa)::value;
            constexpr int ck = G * a;
            z[a] = *reinterpret_cast<const v2f*>(smem_raw + slot_b + lg * 8 + (ck + PADC * (ck / RR)) * 8);
        });
        wave_sync();
        wave_fft<R, C, G>(z, sl, lg, p.tw1, tw2l, [&](auto pp1, int qp, int p2, v2f v) {
            constexpr int p1 = decltype(pp1)::value;
            // window entry of n = qp + R p1 + R^2 p2: mirrored in the upper half when only half the table is kept
            const int n0 = qp + RR * p2;
            float w;
            if constexpr (C > 1) {
                const bool mir = sym && (2 * p2 >= C);
                w = win[(mir ? N - n0 : n0) + (mir ? -R : R) * p1];
            } else {
                w = (p1 < R / 2) ? win[n0 + R * p1] : win[sym ? N - n0 - R * p1 : n0 + R * p1];
            }
            float* dst = pl + qp + (RR + PADP) * p2 + R * p1;
            dst[0] = v.x * w;
            dst[SS] = -(v.y * w);
        });
    }
    XSTAMP(5);   // second transform
    __syncthreads();
    XSTAMP(6);   // barrier
    // ---- overlap-add of the tile's frames: sample i of the segment (clip sample t0 hop - N/2 + i) gathers frames
    // t hop <= i < t hop + N in increasing t; frame t of the tile is the plane at t * SS floats
    const int span = (FPT - 1) * hop + N;
    const long long s0 = (long long)t0 * hop - N / 2;
    float* seg = p.frames + ((size_t)b * tiles + tile) * (size_t)span;
    const float* slf = reinterpret_cast<const float*>(smem_raw);
    // i = t hop + m (0 <= m < hop): frame t is the last one that starts at or before sample i; it and the K - 1 frames before it
    // may cover the sample (at offsets m, m + hop, ...): added in that order.  (t, m) advance by increments, no division per sample.
    const float inv_hop = 1.0f / (float)hop;
    auto div_hop = [&](int v) {                                    // v / hop for 0 <= v < 2^24: float estimate, one correction
        int q = (int)((float)v * inv_hop);
        const int r = v - q * hop;
        q += (r >= hop) ? 1 : 0;
        q -= (r < 0) ? 1 : 0;
        return q;
    };
    const int K = __builtin_amdgcn_readfirstlane(div_hop(N + hop - 1));
    const int qs = __builtin_amdgcn_readfirstlane(div_hop(THREADS)), rs = THREADS - qs * hop;
    const bool all_in = s0 >= 0 && s0 + span <= XG_LC;
    int t = div_hop(tid), m = tid - t * hop;
    float fsum = 0.f;
    for (int i = tid; i < span; i += THREADS) {
        float acc = 0.f;
        int tt = t, off = m;
        for (int kk = 0; kk < K; ++kk) {
            const bool ok = (unsigned)tt < (unsigned)FPT && off < N;
            const int a = tt * SS + off + (PADP ? (off / RR) * PADP : 0);
            const float v = slf[ok ? a : 0];
            acc += ok ? v : 0.f;
            tt -= 1; off += hop;
        }
        seg[i] = acc;
        if (all_in) fsum += acc;
        else { const long long ia = s0 + i; fsum += (ia >= 0 && ia < XG_LC) ? acc : 0.f; }
        m += rs; t += qs;
        if (m >= hop) { m -= hop; t += 1; }
    }
    XSTAMP(7);   // overlap-add, segment stored
    // what the tile contributes to the sum of the clip's gradient (inside the clip): the lanes in a fixed order, the waves in fp64
    fsum = wave_sum(fsum);
    float* red = gm;                                               // (gm is dead)
    if (lane == 0) red[wave] = fsum;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) tot += (double)red[w];
        p.csum[(size_t)b * tiles + tile] = tot;
    }
    XSTAMP(8);   // sum of the tile
}

#undef XG_KERNEL
#undef XG_PARAMS
#undef XG_BO
#undef XG_LC
#undef XG_LENGTHS
#undef XG_PSUM_L
#undef XG_INV_L
#undef XG_TC
#undef XG_GM_END
#undef XG_GM_SAFE
