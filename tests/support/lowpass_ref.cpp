// lowpass_ref.cpp — TEST INFRASTRUCTURE ONLY (tests/test_cuserve_lowpass.py): what the reference's cu[].dct computes once --lowpass-dct has been enabled.
// Built by the test against oracle/_ref/libx265ref{8,10,12}.so and the reference's headers; fills an EncoderPrimitives the way x265_setup_primitives does for a
// C build (setupCPrimitives + setupAliasPrimitives + enableLowpassDCTPrimitives), runs cu[BLOCK_NxN].dct on every block of the input file and prints the
// coefficients.
//   lowpass_ref N FILE        N = 16 | 32; FILE = blocks of N * N int16 (rows contiguous); one line of N * N numbers per block
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "primitives.h"

namespace X265_NS {
void enableLowpassDCTPrimitives(EncoderPrimitives& p);       // primitives.cpp:75 (not declared in primitives.h)
}
using namespace X265_NS;

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s 16|32 blocks.bin\n", argv[0]); return 2; }
    const int n = atoi(argv[1]);
    if (n != 16 && n != 32) { fprintf(stderr, "size %d\n", n); return 2; }
    static EncoderPrimitives p;
    memset(&p, 0, sizeof(p));
    setupCPrimitives(p);
    setupAliasPrimitives(p);
    enableLowpassDCTPrimitives(p);
    const int cu = n == 16 ? BLOCK_16x16 : BLOCK_32x32;
    if (!p.cu[cu].dct || p.cu[cu].dct != p.cu[cu].lowpass_dct || p.cu[BLOCK_8x8].dct == p.cu[BLOCK_8x8].lowpass_dct)
    {
        fprintf(stderr, "the table does not hold the low-pass transforms of sizes 16 and 32 alone\n");
        return 3;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<int16_t> raw(n * n);
    ALIGN_VAR_32(int16_t, src[32 * 32]);
    ALIGN_VAR_32(int16_t, dst[32 * 32]);
    while (fread(raw.data(), sizeof(int16_t), raw.size(), f) == raw.size())
    {
        memcpy(src, raw.data(), sizeof(int16_t) * n * n);
        memset(dst, 0x55, sizeof(dst));
        p.cu[cu].dct(src, dst, n);
        for (int i = 0; i < n * n; i++)
            printf(i ? " %d" : "%d", dst[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
