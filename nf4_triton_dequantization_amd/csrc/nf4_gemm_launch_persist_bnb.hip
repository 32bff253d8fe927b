// nf4_gemm_launch_persist_bnb.hip -- launch_persist_bnb: the launcher of nf4_gemm_launch_persist.hip with the
// bitsandbytes scale modes (nested and single) in place of the reference one, for
// nf4_gemm_bnb / nf4_gemm_bnb_single.  A source of its own so that these instantiations
// compile beside the reference-mode ones.
#define NF4_GEMM_BNB 1
#include "nf4_gemm_launch_persist.hip"
