// mvx_slab_body.inc - one workgroup = one slab: the body shared by voxelize_kernel / voxelize_runs_kernel (float32 grids,
// 64 registers, four 8-wave workgroups per compute unit), voxelize_narrow_kernel (narrow chunks, Ops::NSUB sub-tiles per wave),
// voxelize64_kernel (float64 grids on the matrix cores, 128 registers, two) and voxelize64_vec_kernel (float64 grids on the
// vector ALU). Included inside the kernel definitions, which provide: the type Ops, the constants CT, GROUPED, MAXT and the
// kernel parameters rec, w, slist, slist_ext, Tc, kc, out, P.
// (Textual inclusion, not a __device__ function: with the body in an inlined function template the per-lane-range
// 32-channel variant kept its accumulators in scratch - 193 spilled registers against 4 - whatever the parameter passing.)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = P.NW;             // sub-tiles per slab: z0, the rows of a round, the lane context
    const int NWV = NW / Ops::NSUB;  // waves per workgroup (one sub-tile each but for the narrow kernels): the staging's shares
    unsigned *un = reinterpret_cast<unsigned *>(smem);

    // grid = (T, Z): t = slab id, z = (molecule - b0) * ncc + channel chunk
    unsigned t = blockIdx.x;
    // Which slabs run side by side (blocks are dealt round-robin over the 8 XCDs, ~1000 resident at a time). Grids with
    // several slabs per row (D > 64: a slab is half a 512-B row at D = 128): consecutive blocks take consecutive x-slabs -
    // the resident workgroups then write pieces of every (channel, x) plane instead of filling 32 x planes densely: cfg-5
    // x 8 0.676 -> 0.693 of peak, one cfg-5 call 61.8 -> 61.3 us (same box, twice). Measured and rejected there: the two
    // halves of a row on blocks k and k + 8 (same XCD) 0.58; y fastest 0.56; 8 / 16 x-slabs side by side, then z, y:
    // 0.694 / 0.668; x fastest, then y, then the z chunk 0.703-0.708 (a tie with the order kept); every second x-slab
    // fastest 0.689. Grids of one slab per row (D <= 64) keep z, y, x order: x-slabs fastest costs cfg-2 8 % (0.70).
    unsigned TS = P.nslab; // slabs per molecule (= gridDim.x but for the XCD-range launches)
    bool xcd_ranges = false;
    if constexpr (Ops::RUNS) {
        // Grids written by store_runs (rows that are not whole 16-byte quads): neighbouring slabs share the cache lines at
        // the ends of their runs. Every XCD takes a contiguous range of slabs in z, y, x order (blocks are dealt round-robin
        // over the 8 XCDs; gridDim.x = 8 * ceil(T / 8)), so that the two writers of a line run back to back behind the
        // same L2 and the line goes to memory once.
        if (P.xcd_ranges) {
            const unsigned T = P.nslab, per = gridDim.x >> 3;
            t = (t & 7u) * per + (t >> 3);
            if (t >= T) return;
            xcd_ranges = true;
        }
    }
    if (P.nzc > 1 && !xcd_ranges) { // consecutive blocks = consecutive x-slabs
        const unsigned per_x = (unsigned)(P.nsy * P.nzc), nsx = (unsigned)P.nsx;
        const unsigned tq = __umulhi(t, P.nsx_inv); // t / nsx (nsx > 1 here: several slabs per row means D > 64)
        t = (t - tq * nsx) * per_x + tq;
    }
    int b = (int)blockIdx.y, cc = 0;
    if (P.ncc > 1) {
        b = (int)__umulhi(blockIdx.y, P.ncc_inv); // blockIdx.y / ncc
        cc = (int)blockIdx.y - b * P.ncc;
    }
    b += P.b0;
    // the slab's candidate line: {count, first atom}, then {atom index, packed ranges} per candidate
    const uint2 *__restrict__ line = slist + ((size_t)b * (size_t)TS + t) * SLOTS; // (uniform: scalar loads)
    const uint2 hdr = line[0];
    int sx, sy, zc;
    decode_slab(t, P, sx, sy, zc);
    const int x0 = SUBX * sx, y0 = SUBY * sy, z0 = zc * SUBZ * NW;
    LaneCtx L = Ops::ctx(lane, wave, x0, y0, z0, zc * NW, P.c0 + cc * CT, P);
    if constexpr (GROUPED) {
        // channel-wise radii grouped by radius (chan_aux_kernel): the table of this chunk - the radius slot of this lane's
        // channel, the number of slots, {T, k} of every slot in LDS
        const ChanGroups *__restrict__ G = reinterpret_cast<const ChanGroups *>(Tc) + cc;
        const int *chan_slot = reinterpret_cast<const int *>(kc);
        const int ch = L.cbase + (lane & 31);
        L.grp = ch < P.C ? chan_slot[ch] : -1;
        L.nslots = __builtin_amdgcn_readfirstlane(G->nslots);
        double *gtab = reinterpret_cast<double *>(smem + P.dcap); // (P.dcap: bytes of the rows / tile region in grouped launches)
        if (tid < 2 * CHAN_GROUP_SLOTS) gtab[tid] = reinterpret_cast<const double *>(&G->slot[0])[tid];
        L.gtab = gtab;
        // (published by the staging barrier, which every walk sits behind)
    }

    Ops::tables(L, smem, P, tid); // (float64 matrix-core path: the 2^(j/64) table of exp_nonpos64; published by the staging barrier)

    typename Ops::Acc acc;
    Ops::zero(acc);

    VK_STAMP(0);
    const unsigned n_hdr = __builtin_amdgcn_readfirstlane(hdr.x);
    const int64_t a0 = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane(hdr.y);
    VK_STAMP(1); // the line has arrived
    const int RW = 8 * NW < 64 ? 8 * NW : 64; // rows staged per round
    if (n_hdr > 0) {
        // The normal case is one round over the slab's line (<= 63 candidates, cfg-2: ~45). More candidates than one round
        // of rows (dense slabs: larger radii) take further rounds over the line and its extension, the accumulators carried
        // along. (Round 1 sent such slabs to a second kernel with two workgroups per compute unit: with a 1.5 A radius on
        // cfg-2 that launch took 230 of the step's 618 us.)
        // LINE_OVERFLOW - more candidates than line + extension hold (dense clusters; never at protein densities): the
        // slab's "line" then is the (molecule, x-slab) list itself, any length, in atom order (entry e >= 1 at
        // list[XL_HEADER - 1 + e]): every listed atom's row is staged, and the row filter drops the ones that miss the
        // slab's y rows.
        const bool xl = __builtin_expect(n_hdr > (unsigned)LINE_CAP, 0);
        const uint2 *__restrict__ ext = slist_ext + ((size_t)b * (size_t)TS + t) * EXT_SLOTS;
        int n = (int)n_hdr;
        if (xl) {
            // (xbin_kernel left the list's address in entry 1, for overflowing slabs only. An address rebuilt from loaded
            // words is, to the compiler, a per-lane pointer into any address space: left at that, EVERY line entry of
            // the hot path below is fetched with flat_load through the vector memory pipeline - behind the stores - instead
            // of s_load: cfg-2 x 256 ran at 0.635 of peak against 0.79. Hence the explicit scalar halves and the global
            // address space.)
            const uint2 where = line[1];
            const unsigned long long at = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.y) << 32) |
                                          (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.x);
            typedef const uint2 __attribute__((address_space(1))) *global_u2;
            const global_u2 xlp = (global_u2)at;
            n = __builtin_amdgcn_readfirstlane((int)xlp[0].x);
            line = (const uint2 *)(xlp + (XL_HEADER - 1));
            ext = line + SLOTS;
        }
        // (the first round is peeled: it is staged before the accumulators exist - with 32 accumulators live across the
        // staging loads the kernel needs 90 VGPRs instead of 62 - and the normal case is this one round)
        constexpr bool BIG = MAXT > 512;
        const RoundSrc<Ops> RS_ = round_src<Ops>(rec, w, lane, L, P);
        // (narrow rows - OpsPair - are staged two per load with vector-ALU addresses; written out twice, not as a lambda: the
        // 32-channel kernel then kept ten more registers in scratch)
        if constexpr (Ops::VSTAGE) stage_round_v<Ops, BIG>(line, ext, 0, n, un, rec, w, a0, lane, wave, NWV, RW, L, P);
        else if constexpr (Ops::PRESTAGE) stage_first_rounds<Ops, BIG>(line, ext, n, RW, un, RS_, a0, lane, wave);
        else stage_round<Ops, BIG>(line, ext, 0, n, un, RS_, a0, lane, wave, NW);
        VK_STAMP(2);
        __syncthreads();
        VK_STAMP(3);
        // every further round is staged through registers after the walk before it. (Measured and not kept: the next
        // round's rows by LDS-DMA into a second row buffer while this round is walked - 0.75 / 0.62 / 0.48 of peak at 1.0 /
        // 1.5 / 2.0 A against 0.78 / 0.64 / 0.49; what a compute unit's four workgroups queue on is the vector memory
        // pipeline as a whole, and 27 KB of LDS instead of 18 KB per workgroup costs more than the hidden latency buys.)
        filter_walk<Ops>(xl, acc, 0, n, RW, un, lane, wave, L, P, Tc, kc);
        if (Ops::PRESTAGE && n >= RW) filter_walk<Ops>(xl, acc, RW, n, RW, un + RW * Ops::SW, lane, wave, L, P, Tc, kc); // (staged with the first)
        for (int e0 = Ops::PRESTAGE ? 2 * RW : RW; e0 <= n; e0 += RW) {
            __syncthreads(); // every wave is done with the previous round's rows
            if constexpr (Ops::VSTAGE) stage_round_v<Ops, BIG>(line, ext, e0, n, un, rec, w, a0, lane, wave, NWV, RW, L, P);
            else stage_round<Ops, BIG>(line, ext, e0, n, un, RS_, a0, lane, wave, NW);
            __syncthreads();
            filter_walk<Ops>(xl, acc, e0, n, RW, un, lane, wave, L, P, Tc, kc);
        }
    }
    // 0: empty slab; 1: write-out; 2: write-out of a light slab in a launch of many workgroups - its rounds are paced
    const int write_kind = n_hdr > 0 ? ((P.pace == 2 && n_hdr <= (unsigned)PACE_MAX_CANDIDATES) ? 2 : 1) : 0;
    Ops::write(acc, write_kind, un, tid, lane, wave, NW, b, L, x0, y0, z0, out, P);
    VK_STAMP(6); // all stores issued
#ifdef MVX_DIAG
    if (g_diag && tid == 0) g_diag[16 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + 7] = n_hdr;
#endif
