// union_find_compress.inc -- the compress kernel of union_find.hpp, for inclusion inside namespace hnswgpu's unnamed namespace
// one thread per vertex.  Roots stay roots here: nothing hooks any more.
__global__ __launch_bounds__(256) void cc_compress_kernel(uint32_t* parent, uint32_t n, uint32_t* __restrict__ mark) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = cc_find(parent, v);
    if (r != v) atomicMin(parent + v, r);
    mark[v] = r == v ? 1u : 0u;
}
