// Stand-alone check of clipcap_amd/csrc/cider_table.h (tests/test_cider_ref.py compiles it with the host compiler alone — no HIP include
// path — and once more with -fsanitize=address,undefined): key packing, the hash, the table's build rules, lookups, and a probe chain that
// wraps round the end of the table.
#include <cstdio>
#include <set>
#include <vector>
#include "cider_table.h"

using namespace cc_cider;
static int failures = 0;
#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        if (!(cond)) { failures++; printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

int main() {
    long checked = 0;
    // ---- packing: 16 bits per token, 0xFFFF in the unused slots; unique across n; tokens that cannot be packed give the empty key
    {
        const int toks[] = {0, 1, 2, 40, 65533, 65534};
        std::set<uint64_t> seen;
        long grams = 0;
        for (int n = 1; n <= 4; n++) {
            int idx[4] = {0, 0, 0, 0};
            for (;;) {
                int64_t w[4];
                for (int k = 0; k < n; k++) w[k] = toks[idx[k]];
                const uint64_t key = ct_pack(w, n);
                CHECK(key != CT_EMPTY, "n %d", n);
                for (int k = 0; k < 4; k++)
                    CHECK(((key >> (16 * k)) & 0xFFFF) == (k < n ? (uint64_t)w[k] : 0xFFFFu), "n %d slot %d key %llx", n, k, (unsigned long long)key);
                seen.insert(key);
                grams++;
                int k = 0;
                while (k < n && ++idx[k] == 6) idx[k++] = 0;
                if (k == n) break;
            }
        }
        CHECK((long)seen.size() == grams && grams == 6 + 36 + 216 + 1296, "%zu keys of %ld n-grams", seen.size(), grams);
        const int32_t a[2] = {0, 0}, b[1] = {0};
        CHECK(ct_pack(a, 2) != ct_pack(b, 1) && ct_pack(a, 2) == 0xFFFFFFFF00000000ull && ct_pack(b, 1) == 0xFFFFFFFFFFFF0000ull, "(0, 0) and (0)");
        const int64_t bad1[2] = {5, 65535}, bad2[3] = {-1, 2, 3}, bad3[1] = {int64_t(1) << 40}, bad4[4] = {1, 2, 3, 65536};
        CHECK(ct_pack(bad1, 2) == CT_EMPTY && ct_pack(bad2, 3) == CT_EMPTY && ct_pack(bad3, 1) == CT_EMPTY && ct_pack(bad4, 4) == CT_EMPTY, "unpackable");
        CHECK(ct_pack(bad1, 1) == 0xFFFFFFFFFFFF0005ull, "the tokens beyond n are not looked at");
        checked += grams;
    }
    // ---- the hash: the top log2(cap) bits of key * 0x9E3779B97F4A7C15
    CHECK(ct_log2(1) == 0 && ct_log2(2) == 1 && ct_log2(4096) == 12 && ct_log2(int64_t(1) << 40) == 40, "log2");
    CHECK(ct_pow2(1) && ct_pow2(64) && !ct_pow2(0) && !ct_pow2(-8) && !ct_pow2(48), "pow2");
    for (uint64_t key : {uint64_t(0), uint64_t(1), uint64_t(0xFFFFFFFFFFFF0005ull), uint64_t(0x0001000200030004ull)}) {
        CHECK(ct_slot(key, 0) == 0, "cap 1");
        for (int lg = 1; lg <= 40; lg++) CHECK(ct_slot(key, lg) == (int64_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - lg)), "lg %d", lg);
    }
    // ---- build rules
    {
        std::vector<uint64_t> tk(16);
        std::vector<float> ti(16);
        const uint64_t k8[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        const float f8[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
        CHECK(cider_table_build(k8, f8, 8, tk.data(), ti.data(), 16) == 0, "load 0.5 is allowed");
        CHECK(cider_table_build(k8, f8, 9, tk.data(), ti.data(), 16) == -1, "load above 0.5");
        CHECK(cider_table_build(k8, f8, 4, tk.data(), ti.data(), 12) == -1, "cap not a power of two");
        CHECK(cider_table_build(k8, f8, 0, tk.data(), ti.data(), 0) == -1, "cap 0");
        const uint64_t dup[3] = {7, 8, 7}, emp[2] = {7, CT_EMPTY};
        CHECK(cider_table_build(dup, f8, 3, tk.data(), ti.data(), 16) == -1, "duplicate key");
        CHECK(cider_table_build(emp, f8, 2, tk.data(), ti.data(), 16) == -1, "the empty key");
        CHECK(cider_table_build(nullptr, nullptr, 0, tk.data(), ti.data(), 1) == 0 && tk[0] == CT_EMPTY, "an empty table of one slot");
        CHECK(cider_table_find(tk.data(), ti.data(), 1, 5, -3.f) == -3.f, "a miss in the empty table");
    }
    // ---- every inserted key is found, absent keys and the empty key miss: load exactly 0.5, keys of all four n
    {
        const int64_t cap = 4096, n = cap / 2;
        std::vector<uint64_t> keys;
        std::vector<float> idf;
        uint64_t x = 88172645463325252ull;
        std::set<uint64_t> have;
        while ((int64_t)keys.size() < n) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            int32_t w[4] = {(int32_t)(x & 63), (int32_t)((x >> 8) & 63), (int32_t)((x >> 16) % 65535), (int32_t)((x >> 40) & 63)};
            const uint64_t key = ct_pack(w, 1 + (int)((x >> 60) & 3));
            if (have.insert(key).second) { keys.push_back(key); idf.push_back((float)keys.size()); }
        }
        std::vector<uint64_t> tk(cap);
        std::vector<float> ti(cap);
        CHECK(cider_table_build(keys.data(), idf.data(), n, tk.data(), ti.data(), cap) == 0, "build");
        long used = 0;
        for (uint64_t k : tk) used += k != CT_EMPTY;
        CHECK(used == n, "%ld slots in use", used);
        for (int64_t i = 0; i < n; i++) CHECK(cider_table_find(tk.data(), ti.data(), cap, keys[i], -1.f) == idf[i], "key %lld", (long long)i);
        long misses = 0;
        for (int t = 0; t < 4000; t++) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const uint64_t key = x | 1;                 // any 64-bit pattern
            if (have.count(key) || key == CT_EMPTY) continue;
            CHECK(cider_table_find(tk.data(), ti.data(), cap, key, -7.f) == -7.f, "absent key %llx", (unsigned long long)key);
            misses++;
        }
        CHECK(misses > 3900, "%ld", misses);
        CHECK(cider_table_find(tk.data(), ti.data(), cap, CT_EMPTY, -9.f) == -9.f, "the empty key is never found");
        checked += n + misses;
    }
    // ---- a probe chain that wraps: keys chosen to hash into the second-last slot of a 16-slot table
    {
        const int64_t cap = 16;
        std::vector<uint64_t> keys;
        std::vector<float> idf;
        for (int32_t t = 0; keys.size() < 6 && t < 65535; t++) {
            const uint64_t key = ct_pack(&t, 1);
            if (ct_slot(key, 4) == cap - 2) { keys.push_back(key); idf.push_back(100.f + t); }
        }
        CHECK(keys.size() == 6, "found %zu colliding keys", keys.size());
        uint64_t absent = CT_EMPTY;
        for (int32_t t = 65534; t >= 0; t--) {
            const uint64_t key = ct_pack(&t, 1);
            if (ct_slot(key, 4) == cap - 2 && key != keys.back() && key != keys[0] && key != keys[1] && key != keys[2] && key != keys[3] && key != keys[4]) { absent = key; break; }
        }
        std::vector<uint64_t> tk(cap);
        std::vector<float> ti(cap);
        CHECK(cider_table_build(keys.data(), idf.data(), 6, tk.data(), ti.data(), cap) == 0, "build");
        const int64_t want[6] = {14, 15, 0, 1, 2, 3};
        for (int i = 0; i < 6; i++) {
            CHECK(tk[want[i]] == keys[i], "key %d sits in slot %lld", i, (long long)want[i]);
            CHECK(cider_table_find(tk.data(), ti.data(), cap, keys[i], -1.f) == idf[i], "key %d found round the end", i);
        }
        CHECK(absent != CT_EMPTY && cider_table_find(tk.data(), ti.data(), cap, absent, -2.f) == -2.f, "an absent key walks the whole chain and misses");
        // a full table (not one the builder makes): the probe gives up after cap slots
        for (int64_t s = 0; s < cap; s++) tk[s] = 1000 + (uint64_t)s;
        CHECK(cider_table_find(tk.data(), ti.data(), cap, 5, -4.f) == -4.f, "full table");
        checked += 8;
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok: %ld checks\n", checked);
    return 0;
}
