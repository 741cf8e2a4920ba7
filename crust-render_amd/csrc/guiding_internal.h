// The guiding field's handle between guiding.cpp (the host field, the image, the device copy),
// kernels/guiding_seam.hip (the batched device calls) and render.cpp (crt_renderer_set_guiding). Not part of the ABI.
#pragma once

#include "../../include/crt_guiding.h"
#include "kernels/guiding.hip.h"

namespace crt {

// The device copy of a field's image as the view the kernels take: uploaded on first use, replaced — after waiting for
// the device — when crt_guiding_update has rebuilt the image since. CRT_ERR_NO_DEVICE without a gfx950 device.
int guiding_device(CrtGuiding *g, dev::GuideView &out);

// A holder's reference of its own (a renderer the field is bound to); crt_guiding_free is guiding_release of the
// caller's. The last release waits for the device and frees the device copy.
void guiding_retain(CrtGuiding *g);
void guiding_release(CrtGuiding *g);

}  // namespace crt
