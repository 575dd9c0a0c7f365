// svo_kernels_lk_prior.hip — the motion-prior builds of the LK kernels (k_lk_chain_prior<W>, k_lk_single_guess<W>, W = 5 .. 31) and
// their two launchers: svo_kernels_lk.hip compiled once more with SVO_LK_PRIOR_TU, which swaps that file's host functions and
// launchers for the two *_grid launchers.  A translation unit of its own so that the code object of svo_kernels_lk.hip holds the
// kernels it always held, where it always held them (the comment above the launchers there has the measurement).
#define SVO_LK_PRIOR_TU 1
#include "svo_kernels_lk.hip"
