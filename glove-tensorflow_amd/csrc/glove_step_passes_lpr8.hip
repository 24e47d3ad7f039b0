// sidepass_kernel's builds for the shapes <8, 1> and <8, 2>.
#include "glove_step_passes.h"

namespace glove {

int launch_passes_lpr8(const PassLaunch &a) { return launch_pass_shapes<8, 1, 8, 2>(a); }

#ifdef GLOVE_STAMPS
GLOVE_STAMPS_SETTER(set_stamps_passes_lpr8)
#endif

}  // namespace glove
