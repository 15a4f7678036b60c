// keys.h -- what the key build (keys.hip) and the count stage (dedup.hip) share: the device copy of the key layout and the
// key build as count_records and count_records_sharded call it.
#pragma once

#include "common.h"

struct KL {  // device copy of the layout
    uint32_t sh_umi, sh_lib, sh_feat, sh_bc, bits_umi, bits_lib, bits_feat, bits_bc, umi_len, n_features, n_libs, mux_mask;
    uint32_t bits_ulen, sh_libid, umi_min_len;
};
static KL make_kl(const KeyLayout &L) {
    return KL{L.sh_umi(), L.sh_lib(), L.sh_feat(), L.sh_bc(), L.bits_umi, L.bits_lib, L.bits_feat, L.bits_bc,
              L.umi_len, L.n_features, L.n_libs, L.mux_mask, L.bits_ulen, L.sh_libid(), L.umi_min_len};
}

// The kept reads' keys of `recs` to d_keys_out, their number to *n_keys_out.  d_vals_out (nullable): the read ordinal of every
// key, and the keys then leave in read order (the DupInfo paths).  Defined in keys.hip.
int build_keys_impl(crgpu_ctx *ctx, const crgpu_records *recs, uint64_t *d_keys_out, uint32_t *d_vals_out, uint64_t *n_keys_out);
