// molecule_stages.hip -- the analysis stages that read the molecule table of a crgpu_counts: one translation unit, because
// normalize_depth.h launches the draw kernels of subsample.h and both check their cell lists with the kernel of probe_counts.h.
// Every header names what it uses; the order below is of no consequence.
#include "normalize_depth.h"
#include "probe_counts.h"
#include "subsample.h"
