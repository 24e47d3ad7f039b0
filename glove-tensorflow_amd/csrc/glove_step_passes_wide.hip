// sidepass_kernel's builds for the shapes <64, 3> and <64, 4>.
#include "glove_step_passes.h"

namespace glove {

int launch_passes_wide(const PassLaunch &a) { return launch_pass_shapes<64, 3, 64, 4>(a); }

#ifdef GLOVE_STAMPS
GLOVE_STAMPS_SETTER(set_stamps_passes_wide)
#endif

}  // namespace glove
