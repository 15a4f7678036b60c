// molecule_stages.hip -- the analysis stages that read the molecule table of a crgpu_counts: one translation unit, because
// normalize_depth.h launches the draw kernels of subsample.h.  The barcode segments and the check of a cell list are those of
// stage_common.h; rpu_gmm.h (the enrichment call behind the tallies of feature_metrics.h) rides along.
// Every header names what it uses; the order below is of no consequence.
#include "feature_metrics.h"
#include "normalize_depth.h"
#include "probe_counts.h"
#include "rpu_gmm.h"
#include "subsample.h"
