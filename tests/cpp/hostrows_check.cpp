// Stand-alone host check of rrtmg_lw_amd/csrc/hostrows.hpp - the row scan, the band sum and the row packing of the host-pointer entries -
// on heap buffers of exactly the bytes in use, so that AddressSanitizer sees any access past a row:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rrtmg_lw_amd/csrc tests/cpp/hostrows_check.cpp -o hostrows_check && ./hostrows_check
// (tests/test_hostrows.py builds it plain)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hostrows.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

template <class T>
static void scan_cases()
{
    for (size_t n : {1, 2, 3, 63, 64, 65, 127, 128, 129, 203, 300, 1000}) {
        T *p = static_cast<T *>(std::malloc(n * sizeof(T)));          // (exactly n values: a read of p[n] is a heap overflow)
        uint64_t bits = 0;
        for (size_t i = 0; i < n; i++) p[i] = (T)0.25;
        CHECK(hostrows::row_uniform(p, n, &bits));
        CHECK(bits == hostrows::widened_bits(0.25));
        for (size_t at : {n - 1, n / 2, (size_t)64, (size_t)0}) {
            if (at >= n || n == 1) continue;
            for (size_t i = 0; i < n; i++) p[i] = (T)0.25;
            p[at] = (T)0.5;
            CHECK(!hostrows::row_uniform(p, n, &bits));
        }
        if (n >= 2) {                                                     // a,b,a,b,..: one 8-byte pattern when T is float
            for (size_t i = 0; i < n; i++) p[i] = i % 2 ? (T)0.5 : (T)0.25;
            CHECK(!hostrows::row_uniform(p, n, &bits));
        }
        std::free(p);
    }
}

int main()
{
    scan_cases<float>();
    scan_cases<double>();
    {   // a denormal float widens to the double of the same value; -0.0 and 0.0 are different patterns
        const float den = 1e-40f;
        uint64_t bits = 0;
        CHECK(hostrows::row_uniform(&den, 1, &bits) && bits == hostrows::widened_bits((double)den) && (double)den > 0.0);
        const float z[2] = {0.0f, -0.0f};
        CHECK(!hostrows::row_uniform(z, 2, &bits));
    }
    {   // the band sum: float64 on the widened values, in band order
        float f[16];
        double d[16], want = 0.0;
        for (int i = 0; i < 16; i++) { f[i] = 0.1f * (float)(i + 1) + 1e-7f * (float)i; d[i] = (double)f[i]; want = want + d[i]; }
        CHECK(hostrows::band_sum(f, 16) == want && hostrows::band_sum(d, 16) == want);
    }
    {   // rows of 4-byte values packed at the landing stride and unpacked again: 203 values are 812 bytes, 816 apart
        const size_t w = 203, rows = 7, ncol = 450, st = hostrows::land_stride(w);
        CHECK(st == 816 && hostrows::land_stride(4) == 16 && hostrows::land_stride(5) == 32);
        std::vector<float> src(ncol * rows), back(ncol * rows, -1.0f);
        for (size_t i = 0; i < src.size(); i++) src[i] = (float)i;
        char *packed = static_cast<char *>(std::malloc(st * (rows - 1) + w * 4));          // (the last row ends with its values)
        const size_t col0 = ncol - w;                                                       // (the last columns: the source ends with them)
        hostrows::copy_rows(packed, st, reinterpret_cast<const char *>(src.data() + col0), ncol * 4, w * 4, 0, rows);
        hostrows::copy_rows(reinterpret_cast<char *>(back.data() + col0), ncol * 4, packed, st, w * 4, 0, rows);
        for (size_t r = 0; r < rows; r++)
            for (size_t c = 0; c < ncol; c++) CHECK(back[r * ncol + c] == (c >= col0 ? src[r * ncol + c] : -1.0f));
        std::free(packed);
    }
    std::printf(failures ? "hostrows_check: %d FAILED\n" : "hostrows_check: ok\n", failures);
    return failures ? 1 : 0;
}
