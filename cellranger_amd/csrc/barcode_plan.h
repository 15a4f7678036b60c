// The sizing arithmetic of the barcode stage's host side for a plain C++ program: the constants BIN_SHIFT, BIN_SIZE,
// MB_ITEMS, MB_TILE, MB_MAX_BUCKETS, MB_STAGE_BUDGET, SI_MISS_BUCKET, LH_THREADS, LH_REGIONS, LH_FULL / LH_SPLIT / LH_HOTCNT,
// HC_MAX_RANK_BITS and the functions plan_staging, plan_sampling_batch, plan_miss_record_cap, plan_rank_bits,
// plan_table_mode, plan_table_rounds, plan_k2_sorted.  They are the first section of barcode.hip, which includes nothing
// of HIP up to the end of that section (the reason they are kept there is given at its head); this header stops the
// file at that point.
#pragma once
#define CRGPU_BARCODE_PLAN_ONLY
#include "barcode.hip"
