// fft_block_body.h -- the body of k_fft and k_fft_pix (fft_psd.hip), included between their braces: a workgroup's share of the
// batch, FPB frames at a time.  In scope: the kernel's argument a (FftArgs / FftPixArgs) and the constants N, T, FPB, IN, OUT,
// R0 .. R3, TWG.  (A function that both kernels called would state it as well; k_fft then comes out of the compiler with another
// schedule than it had, and its form was settled by measurement.)
// Where a frame is whole waves (T a multiple of 64) everything this loop hands to fft_fetch / fft_frame about WHICH frame -- the slot
// in the workgroup, the frame's number with the surplus part-workgroup's clamp, the next frame's -- is a scalar: the rows are then
// addressed as scalar base + 32-bit lane offset (wave_row, fft_common.h) and no vector register carries a frame number or an address
// through the passes (profiles/r10_fft_uniform_lanes.md).  Frames of 8 or 16 threads share a wave and keep per-lane values.
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int FE = lds_frame_elems(N);
    constexpr int TWN = TWG ? 0 : tw_total(R0, R1, R2, R3);
    float2 *tw_own = reinterpret_cast<float2 *>(smem);                    // [TWN]
    float2 *bufs = tw_own + TWN;                                          // [FPB][FE]
    float *red_val = reinterpret_cast<float *>(bufs + (size_t)FPB * FE);  // [FPB*NW]
    int *red_idx = reinterpret_cast<int *>(red_val + FPB * ((T + 63) / 64));
    const float2 *tw_lds = TWG ? a.tw : tw_own;
#ifdef JSDR_X_WGCLK
    const unsigned long long wgclk0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long wgclk_n = 0;
#endif

    const int tid_b = threadIdx.x;
    if constexpr (!TWG) {
        for (int i = tid_b; i < TWN; i += T * FPB) tw_own[i] = a.tw[i];
        __syncthreads();
    }

    int fib = tid_b / T;
    const int tid = tid_b - fib * T;
    // whole waves a frame: the slot is a scalar, and so are the frame numbers, the clamp and the row bases made from it below
    if constexpr (frame_is_waves(T)) fib = FPB == 1 ? 0 : __builtin_amdgcn_readfirstlane(fib);
    float2 *buf = bufs + (size_t)fib * FE;
    const long long ngroups = (a.nframes + FPB - 1) / FPB;
    // a surplus part-workgroup (frame count not a multiple of FPB) redoes the last frame: identical values to
    // identical addresses, and no predicate on any load, store or barrier
    auto frame_of = [&](long long g) {
        long long f = g * FPB + fib;
        return f < a.nframes ? f : a.nframes - 1;
    };
    typename RawPoint<IN>::type raw[R0];
    if ((long long)blockIdx.x < ngroups) fft_fetch<N, T, IN, R0>(a, frame_of(blockIdx.x), tid, raw);
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long gn = g + gridDim.x;
        fft_frame<N, T, IN, OUT, R0, R1, R2, R3>(a, frame_of(g), frame_of(gn < ngroups ? gn : g), tid, buf, tw_lds, red_val,
                                                 red_idx, fib, raw);
        __syncthreads();
#ifdef JSDR_X_WGCLK
        wgclk_n++;
#endif
    }
#ifdef JSDR_X_WGCLK
    if (tid_b == 0 && blockIdx.x < WGCLK_WGS) {
        unsigned long long *c = g_fft_wgclk[a.wgclk_slot][blockIdx.x];
        c[0] = wgclk0;
        c[1] = __builtin_amdgcn_s_memrealtime();
        c[2] = wgclk_n;
    }
#endif
