// pf_random.inc -- the counter-based draw of the particle moves (pf_rejuvenate.inc, pf_metropolis.inc; on the host
// sipnet_philox4x32_10, sipnet_rejuvenate_normals, sipnet_mcmc_draws): Philox4x32-10 (Salmon et al. 2011), Box-Muller, the
// four normals of a block, the Metropolis move's partner ranks, and the key of a call.  No generator state anywhere, nothing
// drawn on the host: a word is a function of ctr = {member inside its site, the site's stream, block, draw} and the seed alone,
// so a result depends neither on the number of sites, nor on the path, nor on the launch geometry.
// The block numbers of one member in one draw, and who owns them (two uses must never share a block):
constexpr uint32_t kRejRowBlock = 0;      //  0 ..  3  rejuvenation: the normals of listed rows 4 b .. 4 b + 3
constexpr uint32_t kRejPoolBlock = 4;     //  4 ..  7  rejuvenation: the normals of pools 4 b .. 4 b + 3
constexpr uint32_t kMcBlock = 8;          //  8        Metropolis: partner ranks (words 0, 1), accept uniform (word 2); 9 .. 11 free
constexpr uint32_t kMcJitterBlock = 12;   // 12 .. 15  Metropolis: the jitter's normals of listed rows 4 b .. 4 b + 3

// a call's key: the seed's halves, the draw (the cycle number), and the sites' streams
struct DrawKey {
  uint32_t key0, key1, draw;
  const uint32_t* stream;                  // [n_sites] or null: the site's index
  __device__ __forceinline__ uint32_t streamOf(int s) const { return stream ? stream[s] : (uint32_t)s; }
};
inline DrawKey drawKeyOf(uint64_t seed, uint32_t draw, const uint32_t* d_stream) {
  return DrawKey{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw, d_stream};
}

// Philox4x32-10: ten rounds of two 32 x 32 -> 64 bit products, the key bumped by the Weyl constants between rounds
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}
// a word as a uniform in (0, 1): (x + 0.5) 2^-32, exact
__host__ __device__ inline double uniformOf(uint32_t x) { return ((double)x + 0.5) * 0x1p-32; }
// two normals from two words: u = (xa + 0.5) 2^-32 and v = (xb + 0.5) 2^-32 (exact), r = sqrt(-2 ln u), r cos(2 pi v) and
// r sin(2 pi v).  The angle is reduced exactly -- 2 v = k / 2 + f, |f| <= 1/4 -- before pi enters, so its rounding costs a
// fraction of an ulp instead of 2 pi of them.
__host__ __device__ inline void boxMuller(uint32_t xa, uint32_t xb, double* za, double* zb) {
  const double u = uniformOf(xa), v = uniformOf(xb);
  const double r = sqrt(-2.0 * log(u));
  const int k = (int)rint(4.0 * v);
  const double f = 2.0 * v - 0.5 * (double)k;
#ifdef __HIP_DEVICE_COMPILE__
  const double sf = sinpi(f), cf = cospi(f);
#else
  const double sf = sin(3.14159265358979323846 * f), cf = cos(3.14159265358979323846 * f);
#endif
  const double c = (k & 1) ? ((k & 2) ? sf : -sf) : ((k & 2) ? -cf : cf);
  const double s = (k & 1) ? ((k & 2) ? -cf : cf) : ((k & 2) ? -sf : sf);
  *za = r * c;
  *zb = r * s;
}
// the four normals of one block of one member (second == false: only the first two)
__host__ __device__ inline void memberNormals(const DrawKey& key, uint32_t stream, uint32_t member, uint32_t block, bool second,
                                              double z[4]) {
  uint32_t x[4];
  philox4x32_10(member, stream, block, key.draw, key.key0, key.key1, x);
  boxMuller(x[0], x[1], &z[0], &z[1]);
  if (second) boxMuller(x[2], x[3], &z[2], &z[3]);
}
// the Metropolis move's words of a member: the two partner ranks among nB (0 <= i1, i2 < nB, i1 != i2) and the accept step's word
__host__ __device__ inline void mcDraws(const DrawKey& key, uint32_t stream, uint32_t member, uint32_t nB, int32_t* i1, int32_t* i2,
                                        uint32_t* x2) {
  uint32_t x[4];
  philox4x32_10(member, stream, kMcBlock, key.draw, key.key0, key.key1, x);
  const uint32_t a = (uint32_t)(((uint64_t)x[0] * nB) >> 32);
  uint32_t b = (uint32_t)(((uint64_t)x[1] * (nB - 1u)) >> 32);
  b += b >= a ? 1u : 0u;
  *i1 = (int32_t)a;
  *i2 = (int32_t)b;
  *x2 = x[2];
}
