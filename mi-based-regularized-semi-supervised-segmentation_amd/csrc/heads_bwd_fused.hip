// Fused backward of the local head on 16-bit storage (heads.h has the file map).
#include "heads_bwd_fused.h"

namespace miseg {

int launch_head_bwd_fused(const HeadBwdFused& a) { return launch_head_bwd_fused_t<bf16>(a); }

}  // namespace miseg
