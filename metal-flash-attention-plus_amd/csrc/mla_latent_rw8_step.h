// mla_latent_rw8_step.h — one step of mfa_mla_latent_paged_rw8_kernel's key loop
// (attention_mla_latent_rw8.hip), as text: the loop is unrolled by two by hand so that the
// staging register sets are named statically, and both copies are this file.
//
// Not a stand-alone header.  Contract of the place that includes it:
//   * everything mla_latent_tile_body.h asks for, with `t` the first key of the tile in LDS
//     buffer `cur`;
//   * RW8_HOLD, the staging set that holds tile t + BK (stored to the other LDS buffer when this
//     tile's arithmetic is done), and RW8_FILL, the set that receives tile t + PF·BK now — the
//     same set at prefetch distance 1; both undefined here;
//   * `en[k]`, the block-table entry of tile t + (k + 1)·BK, k <= PF, which the step shifts by
//     one tile; with ROPE, `krf` / `qrf` and the rope lambdas of the rope kernel.
    {
      const bool has_next = t + BK < kend;
      // With ROPE the rope k-step opens the tile's partial Sᵀ (the rope kernel's order).
      f32x16 sp_rope = zero16();
      if constexpr (ROPE) sp_rope = A::mma(krf, qrf, zero16());
      if (t + PF * BK < kend) load(RW8_FILL, t + PF * BK, en[PF - 1]);
      // Scalar work only; without a next tile the buffer is empty and the request a no-op.
      [[maybe_unused]] const __amdgpu_buffer_rsrc_t rrs_next =
          rope_rsrc(t + BK, en[0], ROPE && has_next);
#pragma unroll
      for (int k = 0; k < PF; ++k) en[k] = en[k + 1];
      en[PF] = entry(t + (PF + 2) * BK);
      const char* kt = tb0 + cur * TILEB;

#define MLA_TILE_LEN len
#define MLA_TILE_KLIM klim
#define MLA_TILE_ROPE_SP sp_rope
#define MLA_TILE_ROPE_FETCH()                  \
  if constexpr (ROPE) {                        \
    asm volatile("" : "+v"(s) : : "memory");   \
    krf = rope_load(rrs_next);                 \
  }
#include "mla_latent_tile_body.h"
      if (has_next) store(RW8_HOLD, tb0 + (cur ^ 1) * TILEB);
      __syncthreads();
      cur ^= 1;
    }
#undef RW8_HOLD
#undef RW8_FILL
