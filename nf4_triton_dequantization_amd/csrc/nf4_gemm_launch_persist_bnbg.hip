// nf4_gemm_launch_persist_bnbg.hip -- launch_persist_bnbg: the launcher of nf4_gemm_launch_persist.hip with the
// grouped form of the bitsandbytes scale modes (each weight of the launch with its own
// code2, offset and block sizes), for nf4_gemm_bnb_grouped.  A source of its own so that
// these instantiations compile beside the others.
#define NF4_GEMM_BNBG 1
#include "nf4_gemm_launch_persist.hip"
