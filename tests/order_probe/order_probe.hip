// order_probe.hip -- test-only: vr::order_blocks_kernel (csrc/vr_frame.h) on records the test makes, launched exactly as finish_slot
// launches it behind a march launch -- one workgroup of 1024 threads -- with what it reports read back (tests/test_launch_records_gpu.py).
// Built at test time with build.py's flags into tests/_build/.
#include "vr_frame.h"

#include <cstring>

namespace {

struct Bufs {
    unsigned long long* d_in = nullptr;
    unsigned* d_order = nullptr;
    unsigned* d_heads = nullptr;
    unsigned long long* h_words = nullptr;  // pinned, as the context's: [0] span, [1] end, [2] chain (low word)
    ~Bufs()
    {
        (void)hipFree(d_in);
        (void)hipFree(d_order);
        (void)hipFree(d_heads);
        (void)hipHostFree(h_words);
    }
};

constexpr int kGuard = 64;    // words behind the order that must stay as they were
constexpr int kHeads = 8 * 64;  // a record slot's queue heads: eight, 64 words apart

}  // namespace

#define OP_HIP(x)                         \
    do {                                  \
        const hipError_t e_ = (x);        \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

extern "C" {

int order_probe_max_blocks(void) { return vr::kOrderMaxBlocks; }

// records: n_blocks x kBlockRecord words.  order: n_blocks + 64 words, in and out (the last 64 are the guard).  heads: 512 words, in and
// out (the kernel gets them only with_heads).  words: span, end, chain as the kernel left them -- preset to `preset` (the context zeroes
// them before the launch); the end only with_end.  Returns 0, a HIP error, or -1 for a launch the context would never make.
int order_probe(const unsigned long long* records, int n_blocks, int with_heads, int with_end, unsigned* order, unsigned* heads,
                unsigned long long words[3], unsigned long long preset)
{
    if (n_blocks <= 0 || n_blocks > vr::kOrderMaxBlocks || n_blocks % 8 != 0) return -1;  // (enqueue_render: `ordered`)
    Bufs b;
    const size_t rec_bytes = (size_t)n_blocks * vr::kBlockRecord * sizeof(unsigned long long);
    const size_t ord_bytes = ((size_t)n_blocks + kGuard) * sizeof(unsigned);
    OP_HIP(hipMalloc((void**)&b.d_in, rec_bytes));
    OP_HIP(hipMalloc((void**)&b.d_order, ord_bytes));
    OP_HIP(hipMalloc((void**)&b.d_heads, kHeads * sizeof(unsigned)));
    OP_HIP(hipHostMalloc((void**)&b.h_words, 3 * sizeof(unsigned long long), hipHostMallocDefault));
    OP_HIP(hipMemcpy(b.d_in, records, rec_bytes, hipMemcpyHostToDevice));
    OP_HIP(hipMemcpy(b.d_order, order, ord_bytes, hipMemcpyHostToDevice));
    OP_HIP(hipMemcpy(b.d_heads, heads, kHeads * sizeof(unsigned), hipMemcpyHostToDevice));
    b.h_words[0] = b.h_words[1] = b.h_words[2] = preset;
    hipLaunchKernelGGL(vr::order_blocks_kernel, dim3(1), dim3(1024), 0, (hipStream_t) nullptr, b.d_in, n_blocks, b.d_order,
                       (unsigned*)(b.h_words + 2), b.h_words + 0, with_heads ? b.d_heads : (unsigned*)nullptr,
                       with_end ? b.h_words + 1 : (unsigned long long*)nullptr);
    OP_HIP(hipGetLastError());
    OP_HIP(hipDeviceSynchronize());
    OP_HIP(hipMemcpy(order, b.d_order, ord_bytes, hipMemcpyDeviceToHost));
    OP_HIP(hipMemcpy(heads, b.d_heads, kHeads * sizeof(unsigned), hipMemcpyDeviceToHost));
    std::memcpy(words, b.h_words, 3 * sizeof(unsigned long long));
    return 0;
}

}  // extern "C"
