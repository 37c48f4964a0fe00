// Force-included (-include) in front of every unit of the GEMM launch recorder (tools/record_gemm_launches.py): the HIP runtime calls the
// GEMM launchers make are redefined so that a host-only build records each launch instead of issuing it.  Nothing here feeds back into a
// launcher's decision: the launch macro only copies what it is given, the other calls return constants (256 CUs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <vector>

namespace cc_rec {
struct Launch {
    const void* stub;
    unsigned grid[3], block[3];
    size_t lds;
    std::vector<long long> shapes;      // 9 values per GemmShape argument: M N K lda ldb k_chunk group_m stagger flags
    std::vector<long long> ints;        // every other integer argument, in order (slice counts and extents of the finish kernels; group tables),
                                        // and the functor's switches where it has them (mode, act, img, acc_init, pre_nt)
};
std::vector<Launch>& log();             // defined by the driver
template <class T, class = void> struct is_shape : std::false_type {};
template <class T> struct is_shape<T, decltype((void)(&T::k_chunk))> : std::true_type {};
template <class T, class = void> struct is_group : std::false_type {};
template <class T> struct is_group<T, decltype((void)(&T::whole))> : std::true_type {};
#define CC_REC_FIELD(F)                                                                                  \
    template <class T, class = void> struct has_##F : std::false_type {};                                \
    template <class T> struct has_##F<T, decltype((void)(&T::F))> : std::true_type {};                   \
    template <class T> inline void field_##F(Launch& l, const T& t) { if constexpr (has_##F<T>::value) l.ints.push_back((long long)t.F); }
CC_REC_FIELD(mode) CC_REC_FIELD(act) CC_REC_FIELD(img) CC_REC_FIELD(acc_init) CC_REC_FIELD(pre_nt)
template <class T> inline void shape(Launch& l, const T& g) {
    for (long long v : {(long long)g.M, (long long)g.N, (long long)g.K, (long long)g.lda, (long long)g.ldb, (long long)g.k_chunk, (long long)g.group_m,
                        (long long)g.stagger, (long long)g.flags}) l.shapes.push_back(v);
}
template <class T> inline void arg(Launch& l, const T& t) {
    if constexpr (is_shape<T>::value) shape(l, t);
    else if constexpr (is_group<T>::value) {
        for (long long v : {(long long)t.n, (long long)t.mode, (long long)t.whole, (long long)t.split, (long long)(t.tail != nullptr)}) l.ints.push_back(v);
        for (int i = 0; i < t.n; i++) {
            shape(l, t.g[i]);
            for (long long v : {(long long)t.first[i], (long long)t.zstride[i], (long long)t.ldc[i]}) l.ints.push_back(v);
        }
        l.ints.push_back(t.first[t.n]);
    } else if constexpr (std::is_integral<T>::value) l.ints.push_back((long long)t);
    else if constexpr (std::is_class<T>::value) { field_mode(l, t); field_act(l, t); field_img(l, t); field_acc_init(l, t); field_pre_nt(l, t); }
}
template <class... Args> inline void launch(const void* stub, dim3 g, dim3 b, size_t lds, hipStream_t, const Args&... args) {
    Launch l{stub, {g.x, g.y, g.z}, {b.x, b.y, b.z}, lds, {}, {}};
    (arg(l, args), ...);
    log().push_back(l);
}
}  // namespace cc_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) cc_rec::launch((const void*)(kernel), grid, block, lds, stream, ##__VA_ARGS__)
#define hipFuncSetAttribute(...) hipSuccess
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipDeviceGetAttribute(p, attr, dev) (*(p) = 256, hipSuccess)
