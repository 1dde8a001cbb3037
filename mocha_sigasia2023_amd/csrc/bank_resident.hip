// The two small kernels of a resident bank (mocha_bank_resident_add / _retire, mocha_api.cpp): the storage, the label tables and the slot
// table of the bank are reserved once; a character is added by row copies, its decoder constants, and these two launches on the caller's
// stream, the publish last - a captured step that is replayed afterwards reads the new tables, nothing in it is baked in.
//
//  mocha_resident_labels   one workgroup: the n int32 labels of the new rows -> one label byte per global row (label & 63; no labels: 0),
//                          one granule word per 16 rows (the OR of their label bits; the extent starts on a granule, so the character's
//                          words are gran[first_row / 16 ...]) and the slot's `any` word (the OR over the character).  16 lanes share a
//                          granule: its word is an OR over those lanes by shuffles, `any` an OR over the workgroup through LDS.  Every
//                          word of the extent is WRITTEN, never OR-ed into: what an earlier character left there is gone.
//  mocha_resident_publish  one workgroup: slot table entry {first row, rows} and gran_start[slot], from kernel arguments, ordinary stores.
//                          rows = 0 retires the slot: the matchers then treat its id as they treat an id outside the table.
#include "kernels.h"

namespace mocha {

static_assert(SEG_GRANULE_ROWS == 16, "16 lanes share a granule word below");

__global__ __launch_bounds__(256) void mocha_resident_labels(const int32_t* __restrict__ labels, long long n, long long first_row,
                                                             unsigned char* __restrict__ label, unsigned long long* __restrict__ gran,
                                                             unsigned long long* __restrict__ any_slot) {
    __shared__ unsigned long long wany[4];
    const int tid = threadIdx.x;
    const long long n16 = (n + SEG_GRANULE_ROWS - 1) / SEG_GRANULE_ROWS * SEG_GRANULE_ROWS;
    unsigned long long mine = 0ull;
    for (long long r0 = 0; r0 < n16; r0 += 256) {              // (uniform trip count: the shuffles below run with the whole wave)
        const long long r = r0 + tid;
        unsigned long long bit = 0ull;
        if (r < n) {
            const int l = labels ? (labels[r] & 63) : 0;
            label[first_row + r] = (unsigned char)l;
            bit = 1ull << l;
        }
        mine |= bit;
        unsigned long long g = bit;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) g |= __shfl_xor(g, o);
        if ((tid & 15) == 0 && r < n16) gran[(first_row + r) / SEG_GRANULE_ROWS] = g;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine |= __shfl_xor(mine, o);
    if ((tid & 63) == 0) wany[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) *any_slot = (wany[0] | wany[1]) | (wany[2] | wany[3]);
}

__global__ __launch_bounds__(64) void mocha_resident_publish(int* __restrict__ slots, int* __restrict__ gran_start, int slot, int first_row, int rows) {
    if (threadIdx.x != 0) return;
    slots[2 * slot] = first_row;
    slots[2 * slot + 1] = rows;
    gran_start[slot] = first_row / SEG_GRANULE_ROWS;
}

hipError_t launch_resident_labels(const int32_t* labels, int64_t n, int64_t first_row, int64_t capacity_rows, unsigned char* label,
                                  unsigned long long* gran, unsigned long long* any_slot, hipStream_t s) {
    if (n < 1 || first_row < 0 || first_row % SEG_GRANULE_ROWS != 0 || capacity_rows % SEG_GRANULE_ROWS != 0 || first_row > capacity_rows - n ||
        !label || !gran || !any_slot)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_resident_labels, dim3(1), dim3(256), 0, s, labels, (long long)n, (long long)first_row, label, gran, any_slot);
    return hipGetLastError();
}

hipError_t launch_resident_publish(int* slots, int* gran_start, int slot, int n_slots, int64_t first_row, int64_t rows, int64_t capacity_rows,
                                   hipStream_t s) {
    if (!slots || !gran_start || slot < 0 || slot >= n_slots || rows < 0 || first_row < 0 || first_row % SEG_GRANULE_ROWS != 0 ||
        first_row > capacity_rows - rows || capacity_rows > 0x7fffffff)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_resident_publish, dim3(1), dim3(64), 0, s, slots, gran_start, slot, (int)first_row, (int)rows);
    return hipGetLastError();
}

}  // namespace mocha
