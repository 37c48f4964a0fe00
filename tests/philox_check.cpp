// Stand-alone host check of clipcap_amd/csrc/philox.h: the header alone, no HIP include path (which is the proof that it is HIP-free).
// Known answers of Philox4x32-10 and the mapping (seed, step, row, token) -> noise word that gumbel.hip and tests/gumbel_ref.py use.
// Built and run by tests/test_gumbel_ref.py, plainly and with -fsanitize=address,undefined.
#include "philox.h"

#include <cstdio>

static int fails = 0;

static void expect(const char* what, const philox4& got, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t want[4] = {a, b, c, d};
    for (int i = 0; i < 4; i++)
        if (got.w[i] != want[i]) {
            std::printf("FAIL %s word %d: %08x != %08x\n", what, i, got.w[i], want[i]);
            fails++;
        }
}

int main() {
    expect("zeros", philox4x32_10(0, 0, 0, 0, 0, 0), 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u);
    expect("ones", philox4x32_10(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu), 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u,
           0x6d5451fdu);
    expect("pi", philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u), 0xd16cfe09u, 0x94fdccebu, 0x5001e420u,
           0x24126ea1u);
    // the noise words: counter (token >> 2, row, step, 0), key (lo32(seed), hi32(seed))
    const uint64_t seed = 0x299f31d0a4093822ull;
    const philox4 a = gumbel_bits4(seed, 3, 2, 1), b = philox4x32_10(1, 2, 3, 0, 0xa4093822u, 0x299f31d0u);
    expect("mapping", a, b.w[0], b.w[1], b.w[2], b.w[3]);
    expect("zero seed", gumbel_bits4(0, 0, 0, 0), 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u);
    if (fails) return 1;
    std::printf("ok: philox4x32_10 known answers and the noise-word mapping\n");
    return 0;
}
