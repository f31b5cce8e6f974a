// philox_src.h — Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
// counter-based generator of the sampling kernels (famseq_sample).  ONE definition for both places it runs: compiled into
// capi.cpp (FS_PHILOX_DEF expands to the code; famseq_philox4x32_10 exports it) and carried as text into every generated
// sampling kernel (FS_PHILOX_DEF stringifies it), as phred_src.h is.  Plain C++ only: the 32 x 32 -> 64 products are written as
// unsigned long long, so the text compiles under hiprtc, hipcc and a host compiler alike.
// Ten rounds of  (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key advanced by the
// Weyl constants (W0, W1) after each.  Needs FS_PHILOX_FN, the function's qualifiers.
FS_PHILOX_DEF(
FS_PHILOX_FN void fs_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned *out) {
  for (int r_ = 0; r_ < 10; ++r_) {
    const unsigned long long p0_ = 0xD2511F53ull * (unsigned long long)c0;
    const unsigned long long p1_ = 0xCD9E8D57ull * (unsigned long long)c2;
    const unsigned n0_ = (unsigned)(p1_ >> 32) ^ c1 ^ k0;
    const unsigned n2_ = (unsigned)(p0_ >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1_;
    c3 = (unsigned)p0_;
    c0 = n0_;
    c2 = n2_;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}
)
