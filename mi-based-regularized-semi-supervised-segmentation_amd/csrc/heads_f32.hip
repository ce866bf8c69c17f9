// The local head in exact fp32 (the parity mode): the float instantiations of its forward and fused-backward kernels.  Built once --
// the fp16 build has no such unit (heads.h has the file map).
#include "heads_fwd.h"
#include "heads_bwd_fused.h"

namespace miseg {

int launch_head_fwd_lds_f32(const HeadFwd& a) { return launch_head_fwd_lds<float>(a); }
int launch_head_fwd_reg_f32(const HeadFwd& a, bool quad) { return launch_head_fwd_reg<float>(a, quad); }
int launch_head_bwd_fused_f32(const HeadBwdFused& a) { return launch_head_bwd_fused_t<float>(a); }

}  // namespace miseg
