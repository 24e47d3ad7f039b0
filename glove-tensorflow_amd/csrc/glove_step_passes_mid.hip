// sidepass_kernel's builds for the shapes <32, 3> and <64, 2>.
#include "glove_step_passes.h"

namespace glove {

int launch_passes_mid(const PassLaunch &a) { return launch_pass_shapes<32, 3, 64, 2>(a); }

#ifdef GLOVE_STAMPS
GLOVE_STAMPS_SETTER(set_stamps_passes_mid)
#endif

}  // namespace glove
