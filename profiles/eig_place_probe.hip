// Where do the waves of the batched eigen-solver's workgroups sit?  512 workgroups of 256 threads with group_eig_kernel<2,32>'s
// footprint (224 VGPRs, 15.6 KB of LDS, __launch_bounds__(256, 2): two workgroups per CU, two waves per SIMD).  Every wave
// records its workgroup, its wave number, the hardware-id register (s_getreg HW_REG_HW_ID = 4), the XCC id (register 20) and
// s_memtime at entry and exit; the waves then nap for ~0.1 ms (a fixed count of s_sleep, no waiting on anything), so that
// co-resident workgroups overlap in time.  The host prints
//   * which bits of the register vary, and the value sets of the gfx9 fields (WAVE_ID [3:0], SIMD_ID [5:4], CU_ID [11:8],
//     SH_ID [12], SE_ID [15:13]);
//   * whether the four waves of a workgroup always sit on four different SIMDs, and in which orders;
//   * for every pair of workgroups that overlapped in time on one CU: the SIMDs and slots of their waves 0 and 3.
// Build + run: hipcc --offload-arch=gfx950 -O3 profiles/eig_place_probe.hip -o /tmp/eigprobe && /tmp/eigprobe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <vector>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
struct Rec { unsigned hw, xcc; unsigned long long t0, t1; };
constexpr int NWG = 512;
constexpr int GETREG_HW_ID = 4 | (0 << 6) | (31 << 11);   // id 4, offset 0, 32 bits
constexpr int GETREG_XCC_ID = 20 | (0 << 6) | (31 << 11); // id 20, offset 0, 32 bits
__global__ __launch_bounds__(256, 2) void place_kernel(Rec *__restrict__ out, int naps) {
    __shared__ double lds[1996]; // 15968 bytes, the solver's static LDS
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    const unsigned hw = __builtin_amdgcn_s_getreg(GETREG_HW_ID), xcc = __builtin_amdgcn_s_getreg(GETREG_XCC_ID);
    asm volatile("v_mov_b32 v223, 0" ::: "v223"); // the register file's share of the solver: 224 VGPRs per lane
    for (int i = tid; i < 1996; i += 256) lds[i] = (double)i;
    __syncthreads();
    for (int i = 0; i < naps; i++) __builtin_amdgcn_s_sleep(127);
    __syncthreads();
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) {
        Rec r = {hw, xcc, t0, t1};
        if (lds[wave] < 0.0) r.hw = 0; // (keeps the LDS array)
        out[blockIdx.x * 4 + wave] = r;
    }
}
int main() {
    Rec *d;
    std::vector<Rec> h(NWG * 4);
    CHECK(hipMalloc(&d, h.size() * sizeof(Rec)));
    for (int rep = 0; rep < 2; rep++) { // the first launch warms up
        CHECK(hipMemset(d, 0, h.size() * sizeof(Rec)));
        hipLaunchKernelGGL(place_kernel, dim3(NWG), dim3(256), 0, 0, d, 30);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }
    CHECK(hipMemcpy(h.data(), d, h.size() * sizeof(Rec), hipMemcpyDeviceToHost));
    unsigned all_or = 0, all_and = ~0u;
    std::set<unsigned> waveid, simd, cu, sh, se, xcc;
    for (const Rec &r : h) {
        all_or |= r.hw; all_and &= r.hw;
        waveid.insert(r.hw & 15); simd.insert((r.hw >> 4) & 3); cu.insert((r.hw >> 8) & 15); sh.insert((r.hw >> 12) & 1);
        se.insert((r.hw >> 13) & 7); xcc.insert(r.xcc & 15);
    }
    printf("HW_ID bits that vary over %d waves: 0x%08x (or 0x%08x, and 0x%08x)\n", NWG * 4, all_or & ~all_and, all_or, all_and);
    auto show = [](const char *n, const std::set<unsigned> &s) { printf("  %s:", n); for (unsigned v : s) printf(" %u", v); printf("\n"); };
    show("WAVE_ID [3:0]", waveid); show("SIMD_ID [5:4]", simd); show("CU_ID [11:8]", cu); show("SH_ID [12]", sh);
    show("SE_ID [15:13]", se); show("XCC_ID (reg 20) [3:0]", xcc);
    printf("first 8 workgroups, waves 0..3 as simd.slot (cu key = xcc/se/sh/cu):\n");
    auto cukey = [&](const Rec &r) { return ((r.xcc & 15) << 16) | (r.hw & 0xff00); };
    for (int g = 0; g < 8; g++) {
        printf("  wg %3d key %05x:", g, cukey(h[g * 4]));
        for (int w = 0; w < 4; w++) printf(" %u.%u", (h[g * 4 + w].hw >> 4) & 3, h[g * 4 + w].hw & 15);
        printf("\n");
    }
    int distinct = 0, same_cu = 0, same_slot = 0, same_parity = 0;
    std::map<std::vector<unsigned>, int> orders;
    for (int g = 0; g < NWG; g++) {
        std::set<unsigned> s;
        std::vector<unsigned> ord;
        bool cu_ok = true, slot_ok = true, par_ok = true;
        for (int w = 0; w < 4; w++) {
            const Rec &r = h[g * 4 + w];
            s.insert((r.hw >> 4) & 3); ord.push_back((r.hw >> 4) & 3);
            cu_ok &= cukey(r) == cukey(h[g * 4]);
            slot_ok &= (r.hw & 15) == (h[g * 4].hw & 15);
            par_ok &= (r.hw & 1) == (h[g * 4].hw & 1);
        }
        distinct += s.size() == 4; same_cu += cu_ok; same_slot += slot_ok; same_parity += par_ok;
        orders[ord]++;
    }
    printf("workgroups of %d: four different SIMDs %d, all waves on one CU %d, one slot number in all four waves %d, one slot parity %d\n",
           NWG, distinct, same_cu, same_slot, same_parity);
    printf("SIMD of waves 0,1,2,3 -> workgroups:\n");
    for (auto &kv : orders) printf("  %u %u %u %u : %d\n", kv.first[0], kv.first[1], kv.first[2], kv.first[3], kv.second);
    // pairs of workgroups that overlapped in time on one CU
    std::map<unsigned, std::vector<int>> by_cu;
    for (int g = 0; g < NWG; g++) by_cu[cukey(h[g * 4])].push_back(g);
    printf("CUs that ran workgroups: %zu\n", by_cu.size());
    int pairs = 0, w3_same = 0, w0_same = 0, w03_cross = 0, slot_par_diff = 0, printed = 0;
    std::map<std::pair<unsigned, unsigned>, int> slots;
    for (auto &kv : by_cu)
        for (size_t i = 0; i < kv.second.size(); i++)
            for (size_t j = i + 1; j < kv.second.size(); j++) {
                const int a = kv.second[i], b = kv.second[j];
                const unsigned long long lo = std::max(h[a * 4].t0, h[b * 4].t0), hi = std::min(h[a * 4].t1, h[b * 4].t1);
                if (hi <= lo || 2 * (hi - lo) < h[a * 4].t1 - h[a * 4].t0) continue; // overlapped for at least half a run
                pairs++;
                auto sd = [&](int g, int w) { return (h[g * 4 + w].hw >> 4) & 3; };
                w3_same += sd(a, 3) == sd(b, 3); w0_same += sd(a, 0) == sd(b, 0);
                w03_cross += sd(a, 0) == sd(b, 3) || sd(a, 3) == sd(b, 0);
                slot_par_diff += ((h[a * 4].hw ^ h[b * 4].hw) & 1) != 0;
                slots[{std::min(h[a * 4].hw & 15, h[b * 4].hw & 15), std::max(h[a * 4].hw & 15, h[b * 4].hw & 15)}]++;
                if (printed++ < 12) {
                    printf("  cu %05x: wg %3d", kv.first, a);
                    for (int w = 0; w < 4; w++) printf(" %u.%u", sd(a, w), h[a * 4 + w].hw & 15);
                    printf("  | wg %3d", b);
                    for (int w = 0; w < 4; w++) printf(" %u.%u", sd(b, w), h[b * 4 + w].hw & 15);
                    printf("\n");
                }
            }
    printf("co-resident pairs %d: waves 3 on one SIMD %d, waves 0 on one SIMD %d, a wave 0 with the other's wave 3 %d, slot parity differs %d\n",
           pairs, w3_same, w0_same, w03_cross, slot_par_diff);
    printf("slot numbers (wave 0's) of the two workgroups of a pair -> pairs:\n");
    for (auto &kv : slots) printf("  %u %u : %d\n", kv.first.first, kv.first.second, kv.second);
    CHECK(hipFree(d));
    return 0;
}
