// fit_flow_body.inc -- the body of the undirected persistent fit (kernels_fitp.hip), included by fit_flow_kernel and by
// fit_flow_multi_kernel.  Textual inclusion rather than a __device__ function: the code of fit_flow_kernel's instances stays
// exactly what it was (an inlined function call changes its instruction schedule and register assignment).  The including
// kernel provides TPW, NW, FUSED, NSB, the arguments of fit_flow_kernel by name, and FLOW_WG / FLOW_G: this workgroup's index
// within its problem and the problem's number of workgroups.
    // (4*Nt <= NSB*G, checked by the host)
    __shared__ double red[2][NSB][16][17]; // by the parity of k: no barrier is needed to recycle it
    __shared__ double fred[2][4];
    __shared__ __attribute__((aligned(16))) double tsh[NW][2][64];     // per wave: T of the tile's row block / column block
    // per wave: the two transposing reductions of an iteration ([2][8][FLOW_RLD]); the fused epilogue stages its pieces there
    constexpr int RSH_W = FUSED ? (FLOW_NP * FLOW_RLD > 2 * 8 * FLOW_RLD ? FLOW_NP * FLOW_RLD : 2 * 8 * FLOW_RLD) : 2 * 8 * FLOW_RLD;
    __shared__ __attribute__((aligned(16))) double rsh_all[NW][RSH_W];
    // fused epilogue, filled by the prologue (so the epilogue waits for no global load): per wave the communities of its tile's
    // row / column runs, and {segI, segJ (the rows / columns that start a run, 64-bit masks), fc[I], fc[J], ns[J], base[I][J]}
    static_assert(!FUSED || TPW == 1, "the fused form keeps one tile per wave");
    __shared__ i32 segtab[FUSED ? NW : 1][2][64];
    __shared__ i32 ehdr[FUSED ? NW : 1][8];
    __shared__ int lds_exit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wg = FLOW_WG, G = FLOW_G;
    const int rq = lane >> 3, cq = lane & 7;
    const int NT = Nt * (Nt + 1) / 2;
    const i64 Psz = (i64)Nt * Nt * 64;
    unsigned *fail = sync + 1, *done = sync + 2;
    long long deadline = wall_clock64() + timeout_ticks; // re-armed at every iteration: it bounds one hand-off, not the whole fit

    double g[TPW][8][8];
    int tI[TPW], tJ[TPW];
#ifdef CGE_FLOW_CLOCK
    const long long ck0 = wall_clock64();
#endif
    if (FUSED && (fz.want & 2) && tid < 256) { // the local score's two powers per sample, ahead of everything (nothing is live yet): the
        const cge_fit_fused *ep0 = fz.epi; // epilogue's tally then waits for loads only.  Block vb = this workgroup's, as below
        const i64 S0 = ep0->S;
        const int GR0 = G < 4 * Nt ? G : 4 * Nt;
        if (wg < GR0)
            for (int vb = wg; vb < CGE_PARTIAL_BLOCKS; vb += GR0)
                for (i64 q = (i64)vb * 256 + tid; q < S0; q += (i64)CGE_PARTIAL_BLOCKS * 256) {
                    ep0->apw[q] = pow(1.0 - ep0->dpos[q], fz.alpha);
                    ep0->apw[S0 + q] = pow(1.0 - ep0->dneg[q], fz.alpha);
                }
    }
    if (FUSED && (fz.want & 1)) { // vect_B's tile geometry into LDS (this wave's tile: slot 0)
        const cge_fit_fused *ep0 = fz.epi;
        const int t = wg * NW + wave;
        if (t < NT) { // uniform per wave
            int I = 0, rem = t;
            while (rem >= Nt - I) { rem -= Nt - I; I++; }
            const int J = I + rem;
            const i64 vI = (i64)64 * I + lane, vJ = (i64)64 * J + lane;
            // communities of the block's rows / columns (-1 beyond the matrix): a set bit of segI / segJ starts a run
            const i32 cI = vI < N ? ep0->comm[vI] : -1, cJ = vJ < N ? ep0->comm[vJ] : -1;
            const i32 cIp = __shfl_up(cI, 1), cJp = __shfl_up(cJ, 1);
            const unsigned long long segI = __ballot(lane == 0 || cI != cIp), segJ = __ballot(lane == 0 || cJ != cJp);
            const unsigned long long below = (1ull << lane) - 1ull;
            if ((segI >> lane) & 1ull) segtab[wave][0][__popcll(segI & below)] = cI;
            if ((segJ >> lane) & 1ull) segtab[wave][1][__popcll(segJ & below)] = cJ;
            if (lane == 0) {
                ehdr[wave][0] = (i32)(unsigned)segI; ehdr[wave][1] = (i32)(unsigned)(segI >> 32);
                ehdr[wave][2] = (i32)(unsigned)segJ; ehdr[wave][3] = (i32)(unsigned)(segJ >> 32);
                ehdr[wave][4] = ep0->fc[I]; ehdr[wave][5] = ep0->fc[J]; ehdr[wave][6] = ep0->ns[J]; ehdr[wave][7] = ep0->base[I * Nt + J];
            }
        }
    }
    if (test_naps > 0 && (wg * NW + wave) < NT) // testing (option fit_persistent_test_delay): the tile waves start late
        for (int q = 0; q < test_naps; q++) __builtin_amdgcn_s_sleep(127);
#pragma unroll
    for (int s = 0; s < TPW; s++) {
        const int t = (wg * NW + wave) + s * NW * G;
        tI[s] = -1;
        tJ[s] = -1;
        if (t < NT) {
            int I = 0, rem = t;
            while (rem >= Nt - I) { rem -= Nt - I; I++; }
            tI[s] = I;
            tJ[s] = I + rem;
        }
        if (FUSED) { // the stored logarithm -> this alpha's power, in place (the element stays 0.0 outside the matrix).  Every
            // load is unconditional (indices clamped into the matrix, the result selected afterwards): no divergent branches
            const int Ic = tI[s] < 0 ? 0 : tI[s], Jc = tJ[s] < 0 ? 0 : tJ[s];
            const unsigned Nu = (unsigned)N;
            // The logarithm sits TILE-BLOCKED (k_pow_prepare, blocked form): the 64 doubles (and 64 floats) of a lane's 8 x 8 block are
            // contiguous, a wave's tile is 32 KB (16 KB) of consecutive memory -- 16-byte loads, every line used whole.  (Rounds
            // 4-5 read the row-major matrix: 64 eight-byte loads per lane at a stride of 64 B, 12-26 us of prologue.)
            const size_t tb = ((size_t)(tI[s] < 0 ? 0 : (wg * NW + wave) + s * NW * G) * 64 + (size_t)lane) * 64;
            const dbl2f *bh = reinterpret_cast<const dbl2f *>(fz.Lh + tb);
#pragma unroll
            for (int a = 0; a < 8; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const dbl2f v2 = bh[a * 4 + b];
                    g[s][a][2 * b] = v2.x;
                    g[s][a][2 * b + 1] = v2.y;
                }
            typedef float flt4f __attribute__((ext_vector_type(4)));
            const flt4f *bl = reinterpret_cast<const flt4f *>(fz.Ll + tb);
#pragma unroll
            for (int h = 0; h < 2; h++) { // the float parts by half tiles: 32 registers beside the 128 of the tile
                float ll[4][8];
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const flt4f v4 = bl[(4 * h + a) * 2 + b];
                        ll[a][4 * b] = v4.x; ll[a][4 * b + 1] = v4.y; ll[a][4 * b + 2] = v4.z; ll[a][4 * b + 3] = v4.w;
                    }
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 8; b++) {
                        const bool in = tI[s] >= 0 && 64u * Ic + 8u * rq + 4 * h + a < Nu && 64u * Jc + 8u * cq + b < Nu;
                        const double e = exp2_parts(fz.alpha, g[s][4 * h + a][b], ll[a][b]);
                        g[s][4 * h + a][b] = in ? e : 0.0;
                    }
            }
            continue;
        }
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const i64 row = (i64)64 * tI[s] + 8 * rq + a;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const i64 col = (i64)64 * tJ[s] + 8 * cq + b;
                g[s][a][b] = (tI[s] >= 0 && row < N && col < N) ? GD[row * N + col] : 0.0;
            }
        }
    }
#ifdef CGE_FLOW_CLOCK // (a build flag, diagnostics only: wall-clock stamps of the launch's sections, printed by two waves)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long ck1 = wall_clock64();
#endif
    // the rows this thread updates (threads 0..15 only): the current iterate and the target stay in registers
    const int r16 = tid & 15, qg = (tid >> 4) & 15;
    const bool reducer = tid < 256;
    double tcur[NSB], wrow[NSB];
#pragma unroll
    for (int i = 0; i < NSB; i++) {
        const int sb = wg + i * G;
        const i64 row = (i64)64 * (sb >> 2) + 16 * (sb & 3) + r16;
        const bool mine = sb < 4 * Nt && tid < 16 && row < N;
        tcur[i] = mine ? T0[row] : 0.0;
        wrow[i] = mine ? w[row] : 0.0;
    }
    if (tid == 0) lds_exit = 0;
    __syncthreads();

    int k = 0, converged = 0, failed = 0, left_on = 0;
    if (timeout_ticks <= 0) max_iters = 0; // test hook: abandon at once
    for (;;) {
        deadline = wall_clock64() + timeout_ticks;
        if (k >= max_iters) { failed = 1; break; }
        const double *Tk = (k == 0) ? T0 : ring + (i64)(k & 3) * Tld;
        double *Pk = P + (i64)(k & 1) * Psz;
        int bad = 0; // wave-uniform: 1 = over, 2 = abandoned
        // The arming stores of the previous iteration (and its T) have landed before anything of this iteration is stored:
        // waited for here, where the wave would otherwise only wait for the other workgroups' T to become visible.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // ---- 1. tile products with T_k, each wave on its own -----------------------------------------------------------
#pragma unroll
        for (int s = 0; s < TPW; s++) {
            if (tI[s] < 0 || bad) continue; // uniform per wave
            const int I = tI[s], J = tJ[s];
            double vi, vj;
            unsigned spins = 0;
            for (;;) {
                vi = ld_sc1_at(Tk, 64u * (unsigned)I + (unsigned)lane);
                vj = ld_sc1_at(Tk, 64u * (unsigned)J + (unsigned)lane);
                if (__any(finished_mark(vi) || finished_mark(vj))) { bad = 1; break; } // the fit ended with iteration k - 1
                if (__all(!armed(vi) && !armed(vj))) break;
                bad = flow_check(spins, fail, done, deadline);
                if (bad) break;
            }
            if (bad) continue;
            tsh[wave][0][lane] = vi;
            tsh[wave][1][lane] = vj;
            __builtin_amdgcn_wave_barrier();
            double ti[8], tj[8], pr[8], pc[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                ti[q] = tsh[wave][0][8 * rq + q];
                tj[q] = tsh[wave][1][8 * cq + q];
                pr[q] = 0.0;
                pc[q] = 0.0;
            }
#pragma unroll
            for (int a = 0; a < 8; a++)
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    pr[a] = fma(g[s][a][b], tj[b], pr[a]); // factored: the row's own T_i is applied by the reducer
                    pc[b] = fma(g[s][a][b], ti[a], pc[b]);
                }
            // The transposing reductions of transpose_reduce8 (same pairs, same bits) through LDS: the partial of lane
            // (rq, cq) for row 8*rq + a goes to R[cq][8*rq + a], lane l then adds the eight partials of row l as
            // ((u0+u4)+(u2+u6)) + ((u1+u5)+(u3+u7)); the same for the columns with the roles of rq and cq exchanged.
            double(*R)[FLOW_RLD] = reinterpret_cast<double(*)[FLOW_RLD]>(rsh_all[wave]);
            double(*Cc)[FLOW_RLD] = reinterpret_cast<double(*)[FLOW_RLD]>(rsh_all[wave] + 8 * FLOW_RLD);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                R[cq][8 * rq + q] = pr[q];
                Cc[rq][8 * cq + q] = pc[q];
            }
            __builtin_amdgcn_wave_barrier();
            double u[8], v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                u[q] = R[q][lane];
                v[q] = Cc[q][lane];
            }
            __builtin_amdgcn_wave_barrier();
            const double rsum = ((u[0] + u[4]) + (u[2] + u[6])) + ((u[1] + u[5]) + (u[3] + u[7]));
            st_sc1_at(Pk, ((unsigned)I * (unsigned)Nt + (unsigned)J) * 64u + (unsigned)lane, rsum);
            if (I != J) {
                const double csum = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
                st_sc1_at(Pk, ((unsigned)J * (unsigned)Nt + (unsigned)I) * 64u + (unsigned)lane, csum);
            }
        }
        // ---- 2. the quarter blocks this workgroup reduces -----------------------------------------------------------------
        bool stop = false;
#pragma unroll
        for (int i = 0; i < NSB; i++) {
            const int sb = wg + i * G;
            if (sb >= 4 * Nt) break; // uniform
            const int b = sb >> 2, rib = 16 * (sb & 3) + r16;
            const bool fcheck = k > 0 && i == 0; // `while diff > delta` on f of iteration k-1
            double pv[4] = {0.0, 0.0, 0.0, 0.0}, fv = 0.0, fx[2] = {0.0, 0.0};
            const double *fp = fq + (i64)((k + 2) % 3) * 4 * Nt; // f of iteration k-1
            if (!bad && fcheck && reducer) { // stored an iteration ago: asked for ahead of the partial vectors
#pragma unroll
                for (int u = 0; u < 2; u++)
                    if (tid + 256 * u < 4 * Nt) fx[u] = ld_sc1_at(fp, (unsigned)(tid + 256 * u));
            }
            if (!bad && reducer) {
                unsigned spins = 0;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int q = qg + 16 * u;
                        if (q < Nt) {
                            pv[u] = ld_sc1_at(Pk, ((unsigned)b * (unsigned)Nt + (unsigned)q) * 64u + (unsigned)rib);
                            ok = ok && !armed(pv[u]);
                        }
                    }
                    if (__all(ok)) break;
                    bad = flow_check(spins, fail, done, deadline);
                    if (bad) break;
                }
            }
            if (!bad && fcheck && reducer) {
                unsigned spins = 0;
                for (;;) {
                    if (__all(!armed(fx[0]) && !armed(fx[1]))) break;
                    bad = flow_check(spins, fail, done, deadline);
                    if (bad) break;
#pragma unroll
                    for (int u = 0; u < 2; u++)
                        if (tid + 256 * u < 4 * Nt) fx[u] = ld_sc1_at(fp, (unsigned)(tid + 256 * u));
                }
                fv = fmax(fx[0], fx[1]);
            }
            if (bad && lane == 0) atomicOr(&lds_exit, bad);
            if (reducer) {
                if (fcheck) {
                    fv = wave_max(fv);
                    if (lane == 0) fred[k & 1][wave] = fv;
                }
                red[k & 1][i][qg][r16] = ((pv[0] + pv[1]) + pv[2]) + pv[3];
            }
            __syncthreads();
            const int ex = lds_exit;
            if (ex) { failed = (ex & 2) != 0; converged = !failed; stop = true; break; } // uniform
            if (fcheck) {
                const double f = fmax(fmax(fred[k & 1][0], fred[k & 1][1]), fmax(fred[k & 1][2], fred[k & 1][3]));
                if (!(f > delta)) { // uniform; nothing of iteration k is published -- only the mark that ends the waiting
                    if (tid < 16) {
#pragma unroll
                        for (int i2 = 0; i2 < NSB; i2++) {
                            const int sb2 = wg + i2 * G;
                            if (sb2 < 4 * Nt)
                                st_sc1(ring + (i64)((k + 1) & 3) * Tld + (i64)64 * (sb2 >> 2) + 16 * (sb2 & 3) + r16,
                                       __longlong_as_double((long long)FLOW_FINISHED));
                        }
                    }
                    converged = 1;
                    stop = true;
                    break;
                }
            }
            if (tid < 16) { // the update first: it is what the other workgroups wait for
                double S = red[k & 1][i][0][r16];
#pragma unroll
                for (int u = 1; u < 16; u++) S += red[k & 1][i][u][r16];
                const i64 row = (i64)64 * b + rib;
                double fr = 0.0, tnew = 0.0;
                if (row < N) {
                    S *= tcur[i]; // S_i = T_i * sum_j g_ij T_j: the tiles summed g * T
                    tnew = tcur[i] + (eps * tcur[i]) * (wrow[i] / S - 1.0);
                    fr = fabs(wrow[i] - S);
                }
                st_sc1_at(ring + (i64)((k + 1) & 3) * Tld, (unsigned)row, tnew);
                tcur[i] = tnew;
                fr = row16_max(fr);
                if (r16 == 0) st_sc1_at(fq + (i64)(k % 3) * 4 * Nt, (unsigned)sb, fr);
                st_sc1_at(ring + (i64)((k + 3) & 3) * Tld, (unsigned)row, sentinel());
                if (r16 == 0) st_sc1_at(fq + (i64)((k + 1) % 3) * 4 * Nt, (unsigned)sb, sentinel());
            }
            if (reducer) {
#pragma unroll
                for (int u = 0; u < 4; u++) { // arm the entries just read (their next writer is two iterations away)
                    const int q = qg + 16 * u;
                    if (q < Nt) st_sc1_at(Pk, ((unsigned)b * (unsigned)Nt + (unsigned)q) * 64u + (unsigned)rib, sentinel());
                }
            }
        }
        if (wg >= 4 * Nt && bad) { left_on = bad; break; } // no quarter block, no barrier in the loop: each wave leaves on its own
        if (stop) {
            if (converged && tid == 0) __hip_atomic_store(done, 1u, RLX_AGENT);
            break;
        }
        k++;
    }
    if (converged && tid < 16) { // T_k: every reducer holds its rows
#pragma unroll
        for (int i = 0; i < NSB; i++) {
            const int sb = wg + i * G;
            const i64 row = (i64)64 * (sb >> 2) + 16 * (sb & 3) + r16;
            if (sb < 4 * Nt && row < N) Tout[row] = tcur[i];
        }
    }
    if (wg == 0 && tid == 0) {
        flags[0] = converged;
        flags[1] = k; // iterations done: T_k is final
        flags[2] = failed || !converged;
        flags[3] = 0;
    }
#ifdef CGE_FLOW_CLOCK
    const long long ck2 = wall_clock64();
#endif
    if (!FUSED) return;
    // ---- the rest of the alpha's chain, from the tile and the final iterate --------------------------------------------------
    // A workgroup with a quarter block left the loop as a whole, at iteration k (T_k is final).  A wave of a workgroup without
    // one left on its own when it met the end mark / `done` while polling T_k: for it T_{k-1} is final.  T_final sits in its
    // ring slot, complete and not re-armed: every tile consumed it, and the converging iteration published nothing.
    // (lane ids the compiler cannot see through: nothing of the epilogue is computed ahead of the loop and kept in registers
    // across it -- the loop runs at the 256-register limit)
    int lane_e = lane, tid_e = tid;
    asm volatile("" : "+v"(lane_e), "+v"(tid_e));
    const cge_fit_fused *ep = fz.epi;
    const int want = fz.want;
    const int rq_e = lane_e >> 3, cq_e = lane_e & 7, wave_e = tid_e >> 6;
    const bool wg_reduces = wg < 4 * Nt;
    const bool ok = wg_reduces ? (converged != 0) : (left_on == 1 && k >= 1); // (wave-uniform; an abandoned fit computes nothing)
    const int kfin = wg_reduces ? k : k - 1;
    const double *Tf = (kfin == 0) ? T0 : ring + (i64)(kfin & 3) * Tld;
    if ((want & 1) && ok) {
        double(*R)[FLOW_RLD] = reinterpret_cast<double(*)[FLOW_RLD]>(rsh_all[wave_e]);
        double *const partial = ep->partial; // (the one global load of this part, asked for ahead of the arithmetic)
        {
            constexpr int s = 0;
            if (tI[s] >= 0) { // uniform per wave
            const int I = tI[s], J = tJ[s];
            const unsigned long long segI = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(ehdr[wave_e][1]) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane(ehdr[wave_e][0]);
            const unsigned long long segJ = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(ehdr[wave_e][3]) << 32) |
                                            (unsigned)__builtin_amdgcn_readfirstlane(ehdr[wave_e][2]);
            // T_final of the tile's row and column block: what this wave staged for its last products (tsh is written once per
            // iteration, after the poll that a finished fit never passes)
            double ti[8], tj[8];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                ti[q] = tsh[wave_e][0][8 * rq_e + q];
                tj[q] = tsh[wave_e][1][8 * cq_e + q];
            }
            // (a) pieces: a piece is a run of columns of one community inside this lane_e's 8-column chunk; its eight row sums
            // (ascending column) go to R[piece][row].  pm: the columns that start a piece.
            const unsigned long long pm = segJ | 0x0101010101010101ull;
            const unsigned startb = (unsigned)(pm >> (8 * cq_e)) & 0xFFu, endb = (startb >> 1) | 0x80u;
            int pc = __popcll(pm & ((1ull << (8 * cq_e)) - 1ull));
            double cs[8];
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const bool st = (startb >> b) & 1u;
#pragma unroll
                for (int a = 0; a < 8; a++) {
                    const bool dead = (I == J) && (8 * rq_e + a > 8 * cq_e + b); // the reference sums j >= i only (:229)
                    const double pv = dead ? 0.0 : __dmul_rn(__dmul_rn(ti[a], tj[b]), g[s][a][b]);
                    cs[a] = st ? pv : __dadd_rn(cs[a], pv);
                }
                if ((endb >> b) & 1u) {
#pragma unroll
                    for (int a = 0; a < 8; a++) R[pc][8 * rq_e + a] = cs[a];
                    pc++;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // (b) lane = row: the pieces of a community's run, ascending, into the run's sum -> R[run][row].  All pieces are
            // requested first (the tile's registers are free by now), so the adds do not each wait for an LDS round trip; a lane
            // touches its own column of R only.
            int nrunJ = 0;
            {
                const int npieces = __popcll(pm);
                double xp[FLOW_NP];
#pragma unroll
                for (int q = 0; q < FLOW_NP; q++) xp[q] = q < npieces ? R[q][lane_e] : 0.0;
                unsigned long long m = pm;
                int run = -1;
                double acc = 0.0;
#pragma unroll
                for (int q = 0; q < FLOW_NP; q++) {
                    if (q < npieces) { // uniform
                        const int cpos = __builtin_ctzll(m);
                        m &= m - 1ull;
                        if ((segJ >> cpos) & 1ull) {
                            if (run >= 0) R[run][lane_e] = acc;
                            run++;
                            acc = xp[q];
                        } else
                            acc = __dadd_rn(acc, xp[q]);
                    }
                }
                R[run][lane_e] = acc;
                nrunJ = run + 1;
            }
            __builtin_amdgcn_wave_barrier();
            // (c) lane = column run: the rows of a row run, ascending -> one partial per (row community, column community);
            // again every operand is requested before the first add
            {
                const int run = lane_e < nrunJ ? lane_e : nrunJ - 1;
                const i32 ccol = segtab[wave_e][1][run];
                const bool live = lane_e < nrunJ && ccol >= 0;
                const i32 fcI = __builtin_amdgcn_readfirstlane(ehdr[wave_e][4]), fcJ = __builtin_amdgcn_readfirstlane(ehdr[wave_e][5]),
                          nsJ = __builtin_amdgcn_readfirstlane(ehdr[wave_e][6]);
                double *out = partial + (i64)__builtin_amdgcn_readfirstlane(ehdr[wave_e][7]) + (ccol - fcJ);
                double xr[64];
#pragma unroll
                for (int r = 0; r < 64; r += 2) {
                    const dbl2f v2 = *reinterpret_cast<const dbl2f *>(&R[run][r]);
                    xr[r] = v2.x;
                    xr[r + 1] = v2.y;
                }
                double acc = 0.0;
                int rrun = -1;
                i32 crow = -1;
#pragma unroll
                for (int r = 0; r < 64; r++) { // uniform
                    if ((segI >> r) & 1ull) {
                        if (rrun >= 0 && crow >= 0 && live) out[(i64)(crow - fcI) * nsJ] = acc;
                        rrun++;
                        crow = segtab[wave_e][0][rrun];
                        acc = xr[r];
                    } else
                        acc = __dadd_rn(acc, xr[r]);
                }
                if (crow >= 0 && live) out[(i64)(crow - fcI) * nsJ] = acc;
                // Ids without a member inside a block's range of ids (an empty community between two others): their partials
                // have no term and no run above writes them -- +0.0, as bvec_tile_kernel leaves them, so that the tile's
                // partials are defined whoever made them.  A block's ids are ns = last - first + 1; with as many live runs
                // nothing is missing (uniform: the tiles of a sweep without empty ids never come here).
                const int nrunI = __popcll(segI);
                const int nvI = nrunI - (segtab[wave_e][0][nrunI - 1] < 0 ? 1 : 0), nvJ = nrunJ - (segtab[wave_e][1][nrunJ - 1] < 0 ? 1 : 0);
                const int nsI = segtab[wave_e][0][nvI - 1] - fcI + 1;
                if (nvI != nsI || nvJ != nsJ) {
                    unsigned long long presI = 0ull;
                    for (int u = 0; u < nvI; u++) presI |= 1ull << (segtab[wave_e][0][u] - fcI);
                    bool hasJ = false; // lane = a column id of the block
                    for (int u = 0; u < nvJ; u++) hasJ = hasJ || (segtab[wave_e][1][u] - fcJ == lane_e);
                    double *out0 = partial + (i64)__builtin_amdgcn_readfirstlane(ehdr[wave_e][7]);
                    for (int r = 0; r < nsI; r++)
                        if (lane_e < nsJ && (!((presI >> r) & 1ull) || !hasJ)) out0[(i64)r * nsJ + lane_e] = 0.0;
                }
            }
            }
        }
    }
#ifdef CGE_FLOW_CLOCK
    const long long ck3 = wall_clock64();
#endif
    if ((want & 2) && wg_reduces) { // (`converged` is uniform over such a workgroup: the barriers below are safe)
        double *sh = &rsh_all[0][0]; // >= 256 doubles; every wave_e is past its own use of it once the barrier below is passed
        const int GR = G < 4 * Nt ? G : 4 * Nt;
        __syncthreads();
        for (int vb = wg; vb < CGE_PARTIAL_BLOCKS; vb += GR) { // uniform
            double num = 0.0;
            const i64 S = ep->S;
            if (converged && tid_e < 256)
                for (i64 q = (i64)vb * 256 + tid_e; q < S; q += (i64)CGE_PARTIAL_BLOCKS * 256) {
                    // auc_landmark_kernel's arithmetic on the prepared operands (k_auc_prepare) and this launch's own powers
                    i32 ix[4];
                    double f[8];
#pragma unroll
                    for (int u = 0; u < 4; u++) ix[u] = ep->aidx[u * S + q];
#pragma unroll
                    for (int u = 0; u < 8; u++) f[u] = ep->afac[u * S + q];
                    const double pp = ep->apw[q], pn = ep->apw[S + q], wq = ep->wts[q];
                    const double t_i = ld_sc1(Tf + ix[0]), t_j = ld_sc1(Tf + ix[1]), t_u = ld_sc1(Tf + ix[2]), t_v = ld_sc1(Tf + ix[3]);
                    const double ai = (t_i * f[0]) / f[1], aj = (t_j * f[2]) / f[3];
                    const double au = (t_u * f[4]) / f[5], av = (t_v * f[6]) / f[7];
                    const double pos = (ai * aj) * pp;
                    const double neg = (au * av) * pn;
                    num += (pos > neg ? 1.0 : 0.0) * wq;
                }
            num = flow_sum_256(num, sh, tid_e);
            if (tid_e == 0 && converged) { ep->auc_part[2 * vb] = num; ep->auc_part[2 * vb + 1] = ep->aden[vb]; }
        }
    }
#ifdef CGE_FLOW_CLOCK
    if (lane_e == 0 && ((wg == 0 && wave_e == 0) || (wg == 130 && wave_e == 5)))
        printf("flow clock wg %d wave %d: prologue %lld  loop %lld (%d iterations)  vect_B epilogue %lld  tallies %lld  (10 ns ticks)\n", wg, wave_e,
               ck1 - ck0, ck2 - ck1, k, ck3 - ck2, wall_clock64() - ck3);
#endif
