// mvx_sum_body.inc - the walk of the summed-grid kernels (mvx_sum.hip), textually included into each __global__ as
// mvx_slab_body.inc is: one workgroup per (output slab, chunk of 32 channels) walks the candidate lines of its slab molecule
// after molecule with the accumulators in registers; what becomes of them is the including kernel's last statement.
//
// The including kernel provides: GAUSS, MAXT (template arguments); rec, w, slist, slist_ext, P (kernel arguments); and
//   float *grid       the (C, D, D, D) float32 NCDHW grid this workgroup reads (from_grid) and writes
//   int mol0, nmol    the molecules [mol0, mol0 + nmol) it walks, in order
//   int from_grid     (uniform) the sums start from the values in `grid` instead of zero
// blockIdx.x is the slab, blockIdx.y the channel chunk; blockIdx.z belongs to the including kernel.
    typedef OpsMx32<GAUSS, false, false, false, float> Ops;
    constexpr bool BIG = MAXT > 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = P.NW;
    unsigned *un = reinterpret_cast<unsigned *>(smem);

    // grid = (T, ncc): t = slab id, blockIdx.y = channel chunk
    unsigned t = blockIdx.x;
    const unsigned TS = P.nslab;
    if (P.nzc > 1) { // consecutive blocks = consecutive x-slabs (mvx_slab_body.inc)
        const unsigned per_x = (unsigned)(P.nsy * P.nzc), nsx = (unsigned)P.nsx;
        const unsigned tq = __umulhi(t, P.nsx_inv);
        t = (t - tq * nsx) * per_x + tq;
    }
    const int cc = (int)blockIdx.y;
    int sx, sy, zc;
    decode_slab(t, P, sx, sy, zc);
    const int x0 = SUBX * sx, y0 = SUBY * sy, z0 = zc * SUBZ * NW;
    const LaneCtx L = Ops::ctx(lane, wave, x0, y0, z0, zc * NW, cc * 32, P);

    typename Ops::Acc acc;
    Ops::zero(acc);
    if (from_grid) {
        // read-in, the inverse of OpsMx32::write's map: register r of this lane is channel 8 (r / 4) + 4 (lane / 32) + r % 4 of
        // the chunk at voxel (x0 | x0 + 1, iy, iz). Channels and voxels that do not exist keep their zeros (never written).
        const int D = P.D, h = lane >> 5;
        const size_t D2 = (size_t)D * D, D3 = D2 * D;
        const bool yz = L.iy < D && L.iz < D;
        const bool ok0 = yz && x0 < D, ok1 = yz && x0 + 1 < D;
        const float *src = grid + (size_t)(L.cbase + 4 * h) * D3 + (size_t)x0 * D2 + (size_t)L.iy * D + L.iz;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 8 * (r / 4) + (r % 4);
            if (L.cbase + 4 * h + c < P.C) {
                if (ok0) acc.p0[r] = src[(size_t)c * D3];
                if (ok1) acc.p1[r] = src[(size_t)c * D3 + D2];
            }
        }
    }

    const RoundSrc<Ops> RS_ = round_src<Ops>(rec, w, lane, L, P);
    const int RW = 8 * NW < 64 ? 8 * NW : 64; // rows staged per round
    bool rows_live = false; // (uniform) the row region still holds the rows of the molecule before
    for (int i = 0; i < nmol; ++i) {
        // the candidate line of (molecule mol0 + i, this slab): {count, first atom}, then {atom index, packed ranges} per candidate
        const size_t li = (size_t)(mol0 + i) * (size_t)TS + t;
        const uint2 *__restrict__ line = slist + li * SLOTS; // (uniform: scalar loads)
        const uint2 hdr = line[0];
        const unsigned n_hdr = __builtin_amdgcn_readfirstlane(hdr.x);
        if (n_hdr == 0) continue; // an empty line costs its header: no barrier
        const int64_t a0 = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane(hdr.y);
        const bool xl = __builtin_expect(n_hdr > (unsigned)LINE_CAP, 0); // the slab walks its (molecule, x-slab) list
        const uint2 *__restrict__ ext = slist_ext + li * EXT_SLOTS;
        int n = (int)n_hdr;
        if (xl) { // (explicit scalar halves and the global address space keep every line entry on the scalar path: mvx_slab_body.inc)
            const uint2 where = line[1];
            const unsigned long long at = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.y) << 32) |
                                          (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.x);
            typedef const uint2 __attribute__((address_space(1))) *global_u2;
            const global_u2 xlp = (global_u2)at;
            n = __builtin_amdgcn_readfirstlane((int)xlp[0].x);
            line = (const uint2 *)(xlp + (XL_HEADER - 1));
            ext = line + SLOTS;
        }
        if (rows_live) __syncthreads(); // every wave is done with the rows of the molecule before
        rows_live = true;
        stage_first_rounds<Ops, BIG>(line, ext, n, RW, un, RS_, a0, lane, wave);
        __syncthreads();
        filter_walk<Ops>(xl, acc, 0, n, RW, un, lane, wave, L, P, nullptr, nullptr);
        if (n >= RW) filter_walk<Ops>(xl, acc, RW, n, RW, un + RW * Ops::SW, lane, wave, L, P, nullptr, nullptr); // (staged with the first)
        for (int e0 = 2 * RW; e0 <= n; e0 += RW) {
            __syncthreads();
            stage_round<Ops, BIG>(line, ext, e0, n, un, RS_, a0, lane, wave, NW);
            __syncthreads();
            filter_walk<Ops>(xl, acc, e0, n, RW, un, lane, wave, L, P, nullptr, nullptr);
        }
    }
    // The including kernel ends the walk: MVX_SUM_WRITE (the summed-grid kernels) or an epilogue of its own over acc (mvx_moments.hip:
    // rows_live says whether any line had candidates).
