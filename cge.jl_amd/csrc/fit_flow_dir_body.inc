// fit_flow_dir_body.inc -- the body of the directed persistent fit (kernels_fitp.hip), included by fit_flow_dir_kernel and by
// fit_flow_dir_multi_kernel.  Textual inclusion rather than a __device__ function, as for fit_flow_body.inc: the code of
// fit_flow_dir_kernel's instances stays exactly what it was.  The including kernel provides NW, NSB, the arguments of
// fit_flow_dir_kernel by name, and FLOW_WG / FLOW_G: this workgroup's index within its problem and the problem's number of
// workgroups.
    __shared__ double red[2][NSB][2][16][17]; // [parity of k][quarter block][Sin / Sout]
    __shared__ double fred[2][4];
    __shared__ __attribute__((aligned(16))) double tsh[NW][4][64];          // Tin_I, Tout_I, Tin_J, Tout_J
    __shared__ __attribute__((aligned(16))) double rsh[NW][2][8][FLOW_RLD]; // one pass: a row and a column reduction
    __shared__ int lds_exit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wg = FLOW_WG, G = FLOW_G;
    const int rq = lane >> 3, cq = lane & 7;
    const int NT = Nt * (Nt + 1) / 2;
    const i64 Pstride = (i64)Nt * Nt * 64, Psz = 2 * Pstride;
    unsigned *fail = sync + 1, *done = sync + 2;
    long long deadline = wall_clock64() + timeout_ticks; // re-armed at every iteration: it bounds one hand-off, not the whole fit

    double g[8][8];
    int tI = -1, tJ = -1;
    if (test_naps > 0 && (wg * NW + wave) < NT) // testing (option fit_persistent_test_delay): the tile waves start late
        for (int q = 0; q < test_naps; q++) __builtin_amdgcn_s_sleep(127);
    {
        const int t = wg * NW + wave;
        if (t < NT) {
            int I = 0, rem = t;
            while (rem >= Nt - I) { rem -= Nt - I; I++; }
            tI = I;
            tJ = I + rem;
        }
#pragma unroll
        for (int a = 0; a < 8; a++) {
            const i64 row = (i64)64 * tI + 8 * rq + a;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const i64 col = (i64)64 * tJ + 8 * cq + b;
                g[a][b] = (tI >= 0 && row < N && col < N) ? GD[row * N + col] : 0.0;
            }
        }
    }
    const int r16 = tid & 15, qg = (tid >> 4) & 15;
    const bool reducer = tid < 256;
    double tin_cur[NSB], tout_cur[NSB], din[NSB], dout[NSB];
#pragma unroll
    for (int i = 0; i < NSB; i++) {
        const int sb = wg + i * G;
        const i64 row = (i64)64 * (sb >> 2) + 16 * (sb & 3) + r16;
        const bool mine = sb < 4 * Nt && tid < 16 && row < N;
        tin_cur[i] = mine ? T0[row] : 0.0;
        tout_cur[i] = mine ? T0[Tld + row] : 0.0;
        din[i] = mine ? deg_in[row] : 0.0;
        dout[i] = mine ? deg_out[row] : 0.0;
    }
    if (tid == 0) lds_exit = 0;
    __syncthreads();

    int k = 0, converged = 0, failed = 0;
    double eps = eps0, fprev = f0;
    if (timeout_ticks <= 0) max_iters = 0; // test hook: abandon at once
    for (;;) {
        deadline = wall_clock64() + timeout_ticks;
        if (k >= max_iters) { failed = 1; break; }
        const double *Tk = (k == 0) ? T0 : ring + (i64)(k & 3) * 2 * Tld; // Tin at Tk, Tout at Tk + Tld
        double *Pk = P + (i64)(k & 1) * Psz;
        int bad = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the arming stores of the previous iteration have landed
        // ---- 1. tile products with T_k ---------------------------------------------------------------------------------
        if (tI >= 0) {
            const int I = tI, J = tJ;
            double v0, v1, v2, v3;
            unsigned spins = 0;
            for (;;) {
                v0 = ld_sc1(Tk + 64 * I + lane);
                v1 = ld_sc1(Tk + Tld + 64 * I + lane);
                v2 = ld_sc1(Tk + 64 * J + lane);
                v3 = ld_sc1(Tk + Tld + 64 * J + lane);
                if (__all(!armed(v0) && !armed(v1) && !armed(v2) && !armed(v3))) break;
                bad = flow_check(spins, fail, done, deadline);
                if (bad) break;
            }
            if (!bad) {
                tsh[wave][0][lane] = v0;
                tsh[wave][1][lane] = v1;
                tsh[wave][2][lane] = v2;
                tsh[wave][3][lane] = v3;
                __builtin_amdgcn_wave_barrier();
                const bool diag_tile = I == J;
                double(*R)[FLOW_RLD] = rsh[wave][0];
                double(*Cc)[FLOW_RLD] = rsh[wave][1];
#pragma unroll 1
                for (int pass = 0; pass < 2; pass++) { // one copy of the code: the two passes share their registers
                    // FACTORED (as fit_dataflow_dir_kernel): the row's own factor Tin_i / Tout_i is applied by the reducer.
                    // pass 0: g * Tout -> rows: Sin partial of block I, columns: Sin partial of block J
                    // pass 1: g * Tin  -> rows: Sout partial of block I, columns: Sout partial of block J
                    const double *trow = tsh[wave][1 - pass], *tcol = tsh[wave][3 - pass]; // Tout_I, Tout_J / Tin_I, Tin_J
                    double ta[8], tb[8], pr[8], pc[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        ta[q] = trow[8 * rq + q];
                        tb[q] = tcol[8 * cq + q];
                        pr[q] = 0.0;
                        pc[q] = 0.0;
                    }
#pragma unroll
                    for (int a = 0; a < 8; a++)
#pragma unroll
                        for (int b = 0; b < 8; b++) {
                            double gv = g[a][b];
                            if (diag_tile && rq == cq && a == b) gv += gv; // the j == i term counts twice
                            pr[a] = fma(gv, tb[b], pr[a]);
                            pc[b] = fma(gv, ta[a], pc[b]);
                        }
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
                    // pass 0 -> the Sin plane (0), pass 1 -> the Sout plane (1): rows for block I, columns for block J
                    st_sc1(Pk + (i64)pass * Pstride + ((i64)I * Nt + J) * 64 + lane, rsum);
                    if (!diag_tile) {
                        const double csum = ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
                        st_sc1(Pk + (i64)pass * Pstride + ((i64)J * Nt + I) * 64 + lane, csum);
                    }
                }
            }
        }
        // ---- 2. the quarter blocks this workgroup reduces -----------------------------------------------------------------
        bool stop = false;
#pragma unroll
        for (int i = 0; i < NSB; i++) {
            const int sb = wg + i * G;
            if (sb >= 4 * Nt) break; // uniform
            const int b = sb >> 2, rib = 16 * (sb & 3) + r16;
            const bool fcheck = k > 0 && i == 0;
            double pi[4] = {0.0, 0.0, 0.0, 0.0}, po[4] = {0.0, 0.0, 0.0, 0.0}, fv = 0.0, fx[2] = {0.0, 0.0};
            const double *fp = fq + (i64)((k + 2) % 3) * 4 * Nt; // f of iteration k-1
            if (!bad && fcheck && reducer) {
#pragma unroll
                for (int u = 0; u < 2; u++)
                    if (tid + 256 * u < 4 * Nt) fx[u] = ld_sc1(fp + tid + 256 * u);
            }
            if (!bad && reducer) {
                unsigned spins = 0;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int q = qg + 16 * u;
                        if (q < Nt) {
                            pi[u] = ld_sc1(Pk + ((i64)b * Nt + q) * 64 + rib);
                            po[u] = ld_sc1(Pk + Pstride + ((i64)b * Nt + q) * 64 + rib);
                            ok = ok && !armed(pi[u]) && !armed(po[u]);
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
                        if (tid + 256 * u < 4 * Nt) fx[u] = ld_sc1(fp + tid + 256 * u);
                }
                fv = fmax(fx[0], fx[1]);
            }
            if (bad && lane == 0) atomicOr(&lds_exit, bad);
            if (reducer) {
                if (fcheck) {
                    fv = wave_max(fv);
                    if (lane == 0) fred[k & 1][wave] = fv;
                }
                red[k & 1][i][0][qg][r16] = ((pi[0] + pi[1]) + pi[2]) + pi[3];
                red[k & 1][i][1][qg][r16] = ((po[0] + po[1]) + po[2]) + po[3];
            }
            __syncthreads();
            const int ex = lds_exit;
            if (ex) { failed = (ex & 2) != 0; converged = !failed; stop = true; break; } // uniform
            if (fcheck) { // the step-size rule replayed from the same f history by every workgroup, then `while diff > delta`
                const double f = fmax(fmax(fred[k & 1][0], fred[k & 1][1]), fmax(fred[k & 1][2], fred[k & 1][3]));
                if (f > fprev) eps *= 0.99;
                fprev = f;
                if (!(f > delta)) { converged = 1; stop = true; break; }
            }
            if (tid < 16) {
                double Si = red[k & 1][i][0][0][r16], So = red[k & 1][i][1][0][r16];
#pragma unroll
                for (int u = 1; u < 16; u++) { Si += red[k & 1][i][0][u][r16]; So += red[k & 1][i][1][u][r16]; }
                Si *= tin_cur[i]; // the row's own factor (the tiles summed g * Tout / g * Tin)
                So *= tout_cur[i];
                const i64 row = (i64)64 * b + rib;
                double fr = 0.0, nin = 0.0, nout = 0.0;
                if (row < N) {
                    nin = tin_cur[i];
                    nout = tout_cur[i];
                    if (din[i] > 0) { nin = tin_cur[i] + (eps * tin_cur[i]) * (din[i] / Si - 1.0); fr = fmax(fr, fabs(din[i] - Si)); }
                    if (dout[i] > 0) { nout = tout_cur[i] + (eps * tout_cur[i]) * (dout[i] / So - 1.0); fr = fmax(fr, fabs(dout[i] - So)); }
                }
                double *Tn = ring + (i64)((k + 1) & 3) * 2 * Tld, *Ta = ring + (i64)((k + 3) & 3) * 2 * Tld;
                st_sc1(Tn + row, nin);
                st_sc1(Tn + Tld + row, nout);
                tin_cur[i] = nin;
                tout_cur[i] = nout;
                fr = row16_max(fr);
                if (r16 == 0) st_sc1(fq + (i64)(k % 3) * 4 * Nt + sb, fr);
                st_sc1(Ta + row, sentinel());
                st_sc1(Ta + Tld + row, sentinel());
                if (r16 == 0) st_sc1(fq + (i64)((k + 1) % 3) * 4 * Nt + sb, sentinel());
            }
            if (reducer) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = qg + 16 * u;
                    if (q < Nt) {
                        st_sc1(Pk + ((i64)b * Nt + q) * 64 + rib, sentinel());
                        st_sc1(Pk + Pstride + ((i64)b * Nt + q) * 64 + rib, sentinel());
                    }
                }
            }
        }
        if (wg >= 4 * Nt && bad) break;
        if (stop) {
            if (converged && tid == 0) __hip_atomic_store(done, 1u, RLX_AGENT);
            break;
        }
        k++;
    }
    if (converged && tid < 16) {
#pragma unroll
        for (int i = 0; i < NSB; i++) {
            const int sb = wg + i * G;
            const i64 row = (i64)64 * (sb >> 2) + 16 * (sb & 3) + r16;
            if (sb < 4 * Nt && row < N) {
                Tin_out[row] = tin_cur[i];
                Tout_out[row] = tout_cur[i];
            }
        }
    }
    if (wg == 0 && tid == 0) {
        flags[0] = converged;
        flags[1] = k;
        flags[2] = failed || !converged;
        flags[3] = 0;
    }
