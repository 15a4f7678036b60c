// matrix_stages.hip -- the analysis stages that read a crgpu_matrix_dev: one translation unit, because EmptyDrops and the
// multi-genome bootstrap launch the kernels of the cell call (cell_calling.h).  Every header names what it uses; the order below
// is of no consequence.
#include "aggregates.h"
#include "cell_calling.h"
#include "emptydrops.h"
#include "jibes.h"
#include "kmeans.h"
#include "marginal_calls.h"
#include "matrix_summary.h"
#include "multigenome.h"
#include "perturbations.h"
#include "rtl_tags.h"
#include "sseq.h"
#include "sseq_pair.h"
