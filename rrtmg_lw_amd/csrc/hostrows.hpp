// Host-side row logic of the host-pointer entries (driver.hip: stage_rows, rows_below), free of HIP so that a stand-alone host program
// can exercise it (tools/hostrows_check.cpp).  T is the element type of the caller's array: double, or float in the *_r4 entries.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace hostrows {

template <class T> using Pattern = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;

// the bit pattern of the float64 value the solver reads for v (a float is widened: what k_widen_rows does to the rows that travel)
inline uint64_t widened_bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
inline uint64_t widened_bits(float v) { return widened_bits((double)v); }

// true when the n values at p all hold the bit pattern of p[0] - compared as patterns of sizeof(T) bytes: a float row a,b,a,b,.. is
// uniform to an 8-byte compare and is not uniform.  A row that is not uniform leaves at its first 64 values.  *bits: widened_bits(p[0]).
template <class T>
inline bool row_uniform(const T *p, size_t n, uint64_t *bits)
{
    using U = Pattern<T>;
    const U *u = reinterpret_cast<const U *>(p);
    const U v = u[0];
    U acc = 0;
    size_t i = 0;
    for (; i + 64 <= n && acc == 0; i += 64)
        for (size_t e = 0; e < 64; e++) acc |= u[i + e] ^ v;
    for (; i < n && acc == 0; i++) acc |= u[i] ^ v;
    *bits = widened_bits(p[0]);
    return acc == 0;
}

// tauctot of one cell: the 16 band values of taucld summed in the reference's band order (src/rrtmg_lw_cldprop.f90:173-186), in float64
// on the widened values
template <class T>
inline double band_sum(const T *p, int nbnd)
{
    double sum = 0.0;
    for (int ib = 0; ib < nbnd; ib++) sum = sum + (double)p[ib];
    return sum;
}

// bytes from one float32 row of w values to the next in the landing area and the pinned sets: rows start on 16-byte boundaries
inline size_t land_stride(size_t w) { return (w * 4 + 15) / 16 * 16; }

// `rows` rows of row_bytes each, src_pitch apart at src, to rows dst_pitch apart at dst (packing into the pinned set, unpacking out of it)
inline void copy_rows(char *dst, size_t dst_pitch, const char *src, size_t src_pitch, size_t row_bytes, size_t r0, size_t r1)
{
    for (size_t r = r0; r < r1; r++) std::memcpy(dst + dst_pitch * r, src + src_pitch * r, row_bytes);
}

}   // namespace hostrows
