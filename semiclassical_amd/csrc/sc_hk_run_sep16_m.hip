// The whole-loop kernels of sc_hk_run_m / sc_hk_run_modal_m (per-step second moments of the correlation terms, MOM = true) in a
// translation unit of their own: sc_hk_run_sep16.hip compiled again with SC_RUN_MOMENTS_TU.  Kept apart so that the instantiations
// without moments, which share device helpers with these, are compiled exactly as before.
#define SC_RUN_MOMENTS_TU
#include "sc_hk_run_sep16.hip"
