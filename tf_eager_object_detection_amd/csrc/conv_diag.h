// Host side of the diagnostic build's convolution hooks (include/odet_diag.h), shared by conv3x3.hip, conv_f32.hip and
// conv_x3.hip: every launcher states the plan it is about to launch (ODET_DIAG_PLAN) and keeps its one-time kernel set-up out
// of the way of the plan-only mode (ODET_DIAG_SETUP).  In the shipped library both macros are what the launchers did before:
// nothing, and ODET_HIP(call).
#ifndef ODET_CONV_DIAG_H_
#define ODET_CONV_DIAG_H_
#include "odet_internal.h"

#ifdef ODET_DIAG
#include "../../include/odet_diag.h"

// (defined once, in conv3x3.hip)
bool odet_diag_plan_only();
void odet_diag_record(int family, int form, int nw, int wn, int mt, int ns, int limbs, int ksplit, long long blocks, int forced);

// the record is written whether or not an override is set; in plan-only mode the launcher returns here, before any HIP call
#define ODET_DIAG_PLAN(family, form, nw, wn, mt, ns, limbs, ksplit, blocks, forced)                    \
  do {                                                                                                 \
    odet_diag_record(family, form, nw, wn, mt, ns, limbs, ksplit, (long long)(blocks), (forced) ? 1 : 0); \
    if (odet_diag_plan_only()) return ODET_OK;                                                         \
  } while (0)
#define ODET_DIAG_SETUP(call)                \
  do {                                       \
    if (!odet_diag_plan_only()) ODET_HIP(call); \
  } while (0)
#else
#define ODET_DIAG_PLAN(family, form, nw, wn, mt, ns, limbs, ksplit, blocks, forced) \
  do {                                                                              \
  } while (0)
#define ODET_DIAG_SETUP(call) ODET_HIP(call)
#endif

#endif  // ODET_CONV_DIAG_H_
