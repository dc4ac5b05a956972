// kr_multi_swap.hip -- the two kernels of slot export and import (docs/design/38-slot-swap.md): a staged byte range of a slot image <-> the slot's pages.
// The host cuts the range into pieces (kr_slot_image.h: none crosses a page, none is larger than KR_SLOT_PIECE_CAP); one workgroup moves one piece.  Plain
// streaming copies: 16 bytes per lane and step (the widest global access, 1 KiB per wave instruction) wherever both addresses allow, byte by byte otherwise
// (a flat slot of an odd row size, the 8 bytes of a sampler's state).  No LDS, no scratch, nothing kept between steps: occupancy is bounded by the block size.
#include "kr_multi.h"

// `bytes` bytes from src (null: zeroes) to dst, by the 256 threads of a workgroup
__device__ __forceinline__ void kr_swap_move(char* __restrict__ dst, const char* __restrict__ src, uint32_t bytes) {
    uint32_t done = 0;
    if ((((size_t)dst | (size_t)src) & 15) == 0) {      // a null src is aligned
        const uint32_t n = bytes >> 4;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t i = threadIdx.x; i < n; i += 256) d4[i] = src ? s4[i] : make_uint4(0u, 0u, 0u, 0u);
        done = n << 4;
    }
    for (uint32_t i = done + threadIdx.x; i < bytes; i += 256) dst[i] = src ? src[i] : (char)0;
}

// export: piece blockIdx.x of the range, out of its page into the staging half.  A piece of page -1 (not mapped) writes zeroes
__global__ void __launch_bounds__(256) kr_multi_pack_kernel(const KrPagePoolDev* __restrict__ pools, const KrSlotPiece* __restrict__ pieces, char* __restrict__ stage) {
    const KrSlotPiece pc = pieces[blockIdx.x];
    const KrPagePoolDev P = pools[pc.pool];
    const char* src = pc.page < 0 ? nullptr : (const char*)P.base + (size_t)pc.page * P.page_bytes + pc.page_off;
    kr_swap_move(stage + pc.range_off, src, pc.bytes);
}
// import: the inverse.  It writes the bytes the image holds and no others (what lies behind them in a page was zeroed when the page was mapped); a piece
// without a page has nowhere to go
__global__ void __launch_bounds__(256) kr_multi_unpack_kernel(const KrPagePoolDev* __restrict__ pools, const KrSlotPiece* __restrict__ pieces, const char* __restrict__ stage) {
    const KrSlotPiece pc = pieces[blockIdx.x];
    if (pc.page < 0) return;
    const KrPagePoolDev P = pools[pc.pool];
    kr_swap_move((char*)P.base + (size_t)pc.page * P.page_bytes + pc.page_off, stage + pc.range_off, pc.bytes);
}

void kr_launch_multi_pack(const KrPagePoolDev* pools, const KrSlotPiece* pieces, int n_pieces, void* stage, hipStream_t st) {
    if (n_pieces < 1) return;
    hipLaunchKernelGGL(kr_multi_pack_kernel, dim3(n_pieces), dim3(256), 0, st, pools, pieces, (char*)stage);
}
void kr_launch_multi_unpack(const KrPagePoolDev* pools, const KrSlotPiece* pieces, int n_pieces, const void* stage, hipStream_t st) {
    if (n_pieces < 1) return;
    hipLaunchKernelGGL(kr_multi_unpack_kernel, dim3(n_pieces), dim3(256), 0, st, pools, pieces, (const char*)stage);
}
