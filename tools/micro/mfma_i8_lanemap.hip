// Operand lane map of v_mfma_i32_16x16x64_i8, found with exact integer data (csrc/cindex_boot.hip relies on it).
//   hipcc --offload-arch=gfx950 -O2 tools/micro/mfma_i8_lanemap.hip -o tools/micro/mfma_i8_lanemap && tools/micro/mfma_i8_lanemap
// Each lane holds 16 bytes of A and 16 of B: "slot" (g = lane >> 4, e = byte 0..15) of row / column lane & 15.
//   test 1  A = 1 in slot (g, e) of row r only, B = 1 + 16 g' + e' in every slot of column c: C[r][c] names the B slot that shares A's k.
//           Printed: for every A slot the B slot it pairs with, and whether the pairing is the identity for all 64 slots.
//   test 2  A row r all ones (r = lane & 15), B column c all ones in one column: where in C (lane, register) the value 64 appears.
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef int v4i __attribute__((ext_vector_type(4)));

__global__ void probe(int* pair, int* cpos) {
    const int lane = threadIdx.x, lc = lane & 15, lg = lane >> 4;
    const int r = 5, c = 11;
    for (int slot = 0; slot < 64; ++slot) {
        const int g = slot >> 4, e = slot & 15;
        v4i a = {0, 0, 0, 0}, b = {0, 0, 0, 0}, acc = {0, 0, 0, 0};
        if (lc == r && lg == g) a[e >> 2] = 1 << (8 * (e & 3));
        if (lc == c)
            for (int q = 0; q < 16; ++q) b[q >> 2] |= (1 + 16 * lg + q) << (8 * (q & 3));
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
        // C layout shared by the 16x16 forms: col = lane & 15, row = 4 (lane >> 4) + reg
        if (lc == c && lg == r / 4) pair[slot] = acc[r & 3] - 1;
    }
    for (int rr = 0; rr < 16; ++rr) {
        v4i a = {0, 0, 0, 0}, b = {0, 0, 0, 0}, acc = {0, 0, 0, 0};
        if (lc == rr) a = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
        if (lc == 15 - rr) b = v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
        for (int q = 0; q < 4; ++q)
            if (acc[q] == 64) { cpos[2 * rr] = lane; cpos[2 * rr + 1] = q; }
    }
}

int main() {
    int *pair, *cpos, hp[64], hc[32];
    if (hipMalloc(&pair, sizeof hp) != hipSuccess || hipMalloc(&cpos, sizeof hc) != hipSuccess) return 1;
    if (hipMemset(pair, 0xff, sizeof hp) != hipSuccess || hipMemset(cpos, 0xff, sizeof hc) != hipSuccess) return 1;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, pair, cpos);
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    if (hipMemcpy(hp, pair, sizeof hp, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hc, cpos, sizeof hc, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int identity = 1;
    for (int s = 0; s < 64; ++s) {
        printf("A slot (g %d, e %2d) pairs with B slot (g %d, e %2d)\n", s >> 4, s & 15, hp[s] >> 4, hp[s] & 15);
        identity &= hp[s] == s;
    }
    printf("pairing is the identity: %s\n", identity ? "yes" : "NO");
    int rowcol = 1;
    for (int rr = 0; rr < 16; ++rr) {
        printf("A row lanes &15 == %2d, B column lanes &15 == %2d -> C in lane %2d reg %d (expected lane %2d reg %d)\n", rr, 15 - rr, hc[2 * rr],
               hc[2 * rr + 1], 16 * (rr / 4) + 15 - rr, rr & 3);
        rowcol &= hc[2 * rr] == 16 * (rr / 4) + 15 - rr && hc[2 * rr + 1] == (rr & 3);
    }
    printf("A row = lane & 15, B column = lane & 15, C[4 (lane >> 4) + reg][lane & 15]: %s\n", rowcol ? "yes" : "NO");
    return identity && rowcol ? 0 : 3;
}
