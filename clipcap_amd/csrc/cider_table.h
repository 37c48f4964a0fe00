// The idf table of the CIDEr-D reward (cider.hip): n-gram keys, their hash and an open-addressing table, as plain C++17 with no HIP header.
// The device kernel and the host builder run the same lines (CC_CIDER_HD is __host__ __device__ under hipcc and nothing elsewhere), and
// tests/test_cider_ref.py compiles tests/cider_table_check.cpp against this file with the host compiler alone.
//   key    an n-gram (n = 1..4) of token ids, each in [0, 65535), as one uint64_t: token k in bits [16k, 16k + 16), the unused slots of
//          n < 4 filled with 0xFFFF.  No token is 0xFFFF, so keys are unique across n and all-ones (CT_EMPTY) is no key: it marks an
//          empty slot.  An n-gram with a token outside [0, 65535) cannot be packed: ct_pack gives CT_EMPTY, which ct_find never finds.
//   hash   (key * 0x9E3779B97F4A7C15) >> (64 - log2(cap)): the top log2(cap) bits of the product; cap is a power of two.
//   probe  linear from the hash slot, wrapping at cap, to the key or to the first empty slot; never more than cap slots.
//   table  tab_keys[cap] (CT_EMPTY where empty) and tab_idf[cap]; cider_table_build keeps the load factor at or below 0.5.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CC_CIDER_HD __host__ __device__
#else
#define CC_CIDER_HD
#endif

namespace cc_cider {

constexpr uint64_t CT_EMPTY = ~uint64_t(0);
constexpr uint64_t CT_MUL = 0x9E3779B97F4A7C15ull;
constexpr int CT_TOKEN_LIMIT = 65535;        // token ids of a key lie in [0, CT_TOKEN_LIMIT)
constexpr int CT_NMAX = 4;

CC_CIDER_HD inline bool ct_pow2(int64_t cap) { return cap >= 1 && (cap & (cap - 1)) == 0; }

// key of the n-gram w[0..n), n in 1..4; CT_EMPTY when a token cannot be packed
template <class T>
CC_CIDER_HD inline uint64_t ct_pack(const T* w, int n) {
    uint64_t key = CT_EMPTY;
    for (int k = 0; k < n; k++) {
        const int64_t t = (int64_t)w[k];
        if (t < 0 || t >= CT_TOKEN_LIMIT) return CT_EMPTY;
        key = (key & ~(uint64_t(0xFFFF) << (16 * k))) | ((uint64_t)t << (16 * k));
    }
    return key;
}

CC_CIDER_HD inline int ct_log2(int64_t cap) {          // cap a power of two
    int b = 0;
    while ((int64_t(1) << b) < cap) b++;
    return b;
}

CC_CIDER_HD inline int64_t ct_slot(uint64_t key, int log2cap) { return log2cap ? (int64_t)((key * CT_MUL) >> (64 - log2cap)) : 0; }

// idf of `key`, or `miss` when the table does not hold it
CC_CIDER_HD inline float cider_table_find(const uint64_t* tab_keys, const float* tab_idf, int64_t cap, uint64_t key, float miss) {
    if (key == CT_EMPTY) return miss;
    int64_t s = ct_slot(key, ct_log2(cap));
    for (int64_t probes = 0; probes < cap; probes++) {
        const uint64_t k = tab_keys[s];
        if (k == key) return tab_idf[s];
        if (k == CT_EMPTY) return miss;
        s = (s + 1) & (cap - 1);
    }
    return miss;                                       // a full table without the key (never one that cider_table_build made)
}

// Fills tab_keys[cap] / tab_idf[cap] (host memory) from n distinct keys.  0 = built; -1 = refused, the table's contents then unspecified:
// cap not a power of two, 2 * n > cap (load factor above 0.5), a duplicate key, the empty key.
inline int cider_table_build(const uint64_t* keys, const float* idf, int64_t n, uint64_t* tab_keys, float* tab_idf, int64_t cap) {
    if (!ct_pow2(cap) || n < 0 || n > cap / 2 || (n > 0 && (!keys || !idf)) || !tab_keys || !tab_idf) return -1;
    for (int64_t s = 0; s < cap; s++) { tab_keys[s] = CT_EMPTY; tab_idf[s] = 0.f; }
    const int lg = ct_log2(cap);
    for (int64_t i = 0; i < n; i++) {
        if (keys[i] == CT_EMPTY) return -1;
        int64_t s = ct_slot(keys[i], lg);
        while (tab_keys[s] != CT_EMPTY) {              // ends: at most cap / 2 slots are taken
            if (tab_keys[s] == keys[i]) return -1;
            s = (s + 1) & (cap - 1);
        }
        tab_keys[s] = keys[i];
        tab_idf[s] = idf[i];
    }
    return 0;
}

}  // namespace cc_cider
