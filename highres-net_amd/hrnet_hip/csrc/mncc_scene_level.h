// The body of a level kernel of the tiled masked-NCC search, to be included INSIDE the kernel (after mncc_scene.h): workgroup blockIdx.x
// owns tile `tile` of view `view` and writes its six sums at the P x P grid points of `width` around the centre pair number
// SCENE_LEVEL_CENTRE of `centres` ((0, 0) where `centres` is null) to sums[(blockIdx.x * P^2 + i P + j) * 6 + q].  The kernel has
// scene_level_kernel's parameters and defines SCENE_LEVEL_CENTRE, an expression in `view` and `tile`.  This is text, not a function:
// as an inlined function with its own __restrict__ parameters the same statements get another register allocation, and
// tools/device_code_diff.py holds scene_level_kernel to its code of before the split (as mncc_common.h holds registration.hip's).
    __shared__ SceneShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t view = blockIdx.x / tiles, b = view / V, hw = (size_t)H * W;
    const unsigned tile = blockIdx.x - (unsigned)view * tiles;
    const int ty0 = (int)(tile / tiles_x) * SC_TILE, tx0 = (int)(tile % tiles_x) * SC_TILE;

    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;
        const double c = centres ? (double)centres[2 * (SCENE_LEVEL_CENTRE) + axis] : 0.0;
        split_and_taps(grid_coord(c, width, i, P), &S.whole[axis][i], &S.frac[axis][i], S.tap[axis][i]);
    }
    if (tid == 64) S.mean[0] = plane_mean(means, view, chunks);
    if (tid == 128) S.mean[1] = plane_mean(means, (size_t)BV + b, chunks);
    __syncthreads();
    if (tid < P * P) S.table[tid] = mask_table(S.frac[0][tid / P], S.frac[1][tid % P]);
    const int ny0 = min_whole(S.whole[0], P), nx0 = min_whole(S.whole[1], P);
    stage_window<SC_WIN, SC_WIN>(views + view * hw, view_masks ? view_masks + view * hw : nullptr, S, ty0 + ny0 - 2, tx0 + nx0 - 2, H, W,
                                 S.mean[0], tid);

    // this thread's pixels of the reference, centred on the reference's mean under its own mask and zero where that mask is set
    float r[SC_ITEMS][SC_RUN];
    unsigned rbits = 0;
    const int x = lane, gx = tx0 + x;
    {
        const float* rp = ref + b * hw;
        const float* rm = ref_mask ? ref_mask + b * hw : nullptr;
        const float mean = S.mean[1];
#pragma unroll
        for (int k = 0; k < SC_ITEMS; ++k)
#pragma unroll
            for (int p = 0; p < SC_RUN; ++p) {
                const int gy = ty0 + (wave + k * SC_WAVES) * SC_RUN + p;
                const bool in = gy < H && gx < W;
                const size_t g = in ? (size_t)gy * W + gx : 0;
                const bool m = in && (rm ? rm[g] != 0.f : true);
                r[k][p] = m ? rp[g] - mean : 0.f;
                rbits |= (unsigned)m << (SC_RUN * k + p);
            }
    }

#pragma unroll 1
    for (int j = 0; j < P; ++j) {
        const int nx = S.whole[1][j], offx = nx - nx0;
        const bool jok = offx <= SC_SPAN;
        if (jok) scene_row_pass(S, S.tap[1][j], offx, SC_WIN, tid);
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < P; ++i) {
            const int ny = S.whole[0][i], offy = ny - ny0;
            const unsigned table = S.table[i * P + j];
            float ky[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) ky[o] = S.tap[0][i][o];
            int n = 0;
            double st = 0.0, sr = 0.0, stt = 0.0, srr = 0.0, srt = 0.0;
            if (jok && offy <= SC_SPAN) {
#pragma unroll
                for (int k = 0; k < SC_ITEMS; ++k) {
                    const int yl = (wave + k * SC_WAVES) * SC_RUN;
                    float t[SC_RUN];
                    const unsigned c = scene_column_run(S, ky, ny, nx, offy, offx, table, x, yl, ty0 + yl, gx, H, W, t) & (rbits >> (SC_RUN * k));
                    n += __popc(c & ((1u << SC_RUN) - 1u));
#pragma unroll
                    for (int p = 0; p < SC_RUN; ++p) {
                        const bool on = (c >> p) & 1u;
                        float tf = on ? t[p] : 0.f, rf = on ? r[k][p] : 0.f;
                        asm("" : "+v"(tf), "+v"(rf));    // the selects stay in fp32: one each, not two on the halves of a double
                        const double tm = (double)tf, rm = (double)rf;
                        st += tm; sr += rm;
                        stt = fma(tm, tm, stt); srr = fma(rm, rm, srr); srt = fma(rm, tm, srt);
                    }
                }
            }
            double v[8] = {(double)n, st, sr, stt, srr, srt, 0.0, 0.0};
            WaveSums<8, 0>::run(v, lane);
            if (lane < 8) S.red[i][wave][wave_sums_index<8>(lane)] = v[0];
        }
        __syncthreads();                         // A and S.red are free again after this
        if (tid < P * RG_NSUM) {
            const int i = tid / RG_NSUM, q = tid - i * RG_NSUM;
            double s = 0.0;
            for (int w = 0; w < SC_WAVES; ++w) s += S.red[i][w][q];
            S.tot[i * P + j][q] = s;
        }
    }
    __syncthreads();
    double* out = sums + (size_t)blockIdx.x * (P * P * RG_NSUM);
    const double* tot = &S.tot[0][0];
    for (int i = tid; i < P * P * RG_NSUM; i += SC_THREADS) out[i] = tot[i];
