// sage_kv_append_body.h -- the body of kvcache_append_kernel, kvpaged_append_kernel and kvpvarlen_append_kernel (sage_kv_cache.hip,
// sage_kv_paged.hip, sage_kv_varlen.hip): a code fragment, included INSIDE the three kernel functions with SAGE_KV_APPEND_PAGED defined as
// 0 / 1 / 1 and, by the third alone, SAGE_KV_APPEND_RAGGED as 1 (shared as text: as a function template it gave the unpaged kernels
// other code).  Not a header of its own: no include guard, no declarations.
    constexpr int CPR = D / 16;                 // 16-element chunks per row
    constexpr int NCH = BLKK * CPR / 256;       // chunks per thread
    constexpr int LDT = D + 8;                  // padded row (16-B aligned), as prep_v_kernel
    __shared__ unsigned gmax[4];
    __shared__ __attribute__((aligned(16))) uint16_t tile[BLKK * LDT];

    const int tid = threadIdx.x;
    const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const long bh = (long)b * p.H + h;
    int len0, t;
#if defined(SAGE_KV_APPEND_RAGGED) && SAGE_KV_APPEND_RAGGED      // (packed new rows, sage_kv_varlen.hip: the sample's rows from the prefix array; the preprocessor, as below)
    int new0;                                   // the sample's first row of the packed k_new / v_new
    ragged_append_range(p, r, b, len0, t, new0);
#else
    append_range(p, b, len0, t);
#endif
    // the scales of the frozen abs-max (every call: the same bytes; a sample that never gets a row has them too)
    if (j == 0 && tid < D) p.v_scale[bh * D + tid] = fp8_v_scale(p.v_amax[bh * D + tid], p.scale_max);
    const int len1 = len0 + t;                  // <= cap
    const int blk = len0 / BLKK + j;
    const int row0 = blk * BLKK;
    if (row0 >= len1) return;                   // no new row for this block (t == 0 included); row0 < len1 <= cap: the block exists
    // the block's place: in the sample's own slab, or (PAGED) in the page the table names
#if SAGE_KV_APPEND_PAGED      // (the preprocessor: the unpaged kernel has no second argument to name, and its statements stay as they were written)
    long kv_blk;                                           // the block's index among the 64-row blocks of the pool: (page, head, block of the page)
    {
        const int page = g.block_table[(long)b * g.bt_stride + (blk >> g.page_shift)];      // (blk < cap / 64: an entry of the sample's row)
        if (page < 0 || page >= g.num_pages) return;       // not a page of the pool: nothing of the block is written (lens still advance)
        kv_blk = (((long)page * p.H + h) << g.page_shift) + (blk & ((1 << g.page_shift) - 1));
    }
#endif
    const int valid = len1 - row0 < BLKK ? len1 - row0 : BLKK;
    const int old = len0 - row0;                // rows r < old of the block are the tails' (j = 0), the rest k_new's / v_new's
#if defined(SAGE_KV_APPEND_RAGGED) && SAGE_KV_APPEND_RAGGED
    const uint16_t *k_new = p.k_new + (long)h * p.k_sh + ((long)new0 + (row0 - len0)) * p.k_sl;              // row r of the block (k_sb / v_sb unused)
    const uint16_t *v_new = p.v_new + (long)h * p.v_sh + ((long)new0 + (row0 - len0)) * p.v_sl;
#else
    const uint16_t *k_new = p.k_new + (long)b * p.k_sb + (long)h * p.k_sh + (long)(row0 - len0) * p.k_sl;     // row r of the block
    const uint16_t *v_new = p.v_new + (long)b * p.v_sb + (long)h * p.v_sh + (long)(row0 - len0) * p.v_sl;
#endif
    const uint16_t *k_tail = p.k_tail + bh * (BLKK * D);
    const uint16_t *v_tail = p.v_tail + bh * (BLKK * D);

    if (tid < 4) gmax[tid] = 0u;
    // V rows -> LDS, zero behind the last valid token
    constexpr int TPR = D / 8;
#pragma unroll
    for (int i = 0; i < BLKK * TPR / 256; i++) {
        const int piece = tid + 256 * i;
        const int r = piece / TPR, c8 = (piece % TPR) * 8;
        v4u raw = {0u, 0u, 0u, 0u};
        if (r < valid) raw = *reinterpret_cast<const v4u *>(r < old ? v_tail + r * D + c8 : v_new + (long)r * p.v_sl + c8);
        *reinterpret_cast<v4u *>(&tile[r * LDT + c8]) = raw;
    }
    __syncthreads();

    // ---- INT8 K: quant_int8_kernel for GR_THREAD_K / QS_TRITON_THREAD over the block's valid rows
    const uint16_t *mean = p.k_mean != nullptr ? p.k_mean + bh * D : nullptr;
    float v[NCH][16];
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = tid + 256 * i;
        const int r = c / CPR, col = (c % CPR) * 16;
        if (r < valid) {
            const v4u *src = reinterpret_cast<const v4u *>(r < old ? k_tail + r * D + col : k_new + (long)r * p.k_sl + col);
            v4u raw[2] = {src[0], src[1]};
            v4u mraw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            if (mean != nullptr) {
                const v4u *ms = reinterpret_cast<const v4u *>(mean + col);
                mraw[0] = ms[0];
                mraw[1] = ms[1];
            }
            const float amax = quant_load16<DT>(raw, mraw, mean != nullptr, QS_TRITON_THREAD, 1.0f, v[i]);
            atomicMax(&gmax[group_of_row(r, GR_THREAD_K, BLKK)], __float_as_uint(amax));
        } else {
#pragma unroll
            for (int e = 0; e < 16; e++) v[i][e] = 0.0f;
        }
    }
    __syncthreads();

#if SAGE_KV_APPEND_PAGED
    if (tid < 4) p.k_scale[kv_blk * 4 + tid] = quant_scale(__uint_as_float(gmax[tid]), QS_TRITON_THREAD);
    int8_t *k_out = p.k_int8 + kv_blk * (BLKK * D);
#else
    if (tid < 4) p.k_scale[bh * (p.cap / BLKK * 4) + blk * 4 + tid] = quant_scale(__uint_as_float(gmax[tid]), QS_TRITON_THREAD);
    int8_t *k_out = p.k_int8 + (bh * p.cap + row0) * D;
#endif
#pragma unroll
    for (int i = 0; i < NCH; i++) {
        const int c = tid + 256 * i;
        const int r = c / CPR, col = (c % CPR) * 16;
        if (r >= valid) continue;
        const float am = __uint_as_float(gmax[group_of_row(r, GR_THREAD_K, BLKK)]);
        const v4u pk = quant_pack16(v[i], am, QS_TRITON_THREAD);
        *reinterpret_cast<v4u *>(k_out + r * D + col) = pk;        // (the attention call that follows reads it: no non-temporal hint)
    }

    // ---- FP8 V: the block's whole tile image, prep_v_kernel<.., FP8> with am = v_amax
    const float *amx = p.v_amax + bh * D;
#if SAGE_KV_APPEND_PAGED
    unsigned char *out = p.v_image + kv_blk * (long)(D * 64);
#else
    unsigned char *out = p.v_image + (bh * (p.cap / BLKK) + blk) * (long)(D * 64);
#endif
#pragma unroll
    for (int i = 0; i < D * 4 / 256; i++) {
        const int piece = tid + 256 * i;
        const int d = piece >> 2, pc = piece & 3;
        const v4u pk = fp8_v_image_piece<DT, LDT>(tile, d, pc, 0.0f, fp8_v_recp(amx[d], p.scale_max), false, valid);
        *reinterpret_cast<v4u *>(out + d * 64 + pc * 16) = pk;
    }
