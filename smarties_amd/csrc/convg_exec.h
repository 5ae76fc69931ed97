// smarties_amd/csrc/convg_exec.h -- the launches of a convolutional layer of general geometry (ConvGeo::gen, convg.hip) inside the step's
// launch sequences (included by learner.cpp in front of step_exec.h, whose launchFront / launchBackward call these per layer).  Counters
// of their own, one family per pass: the launch-count tables of the nets that conv.hip serves (tests/blocks.py) list none of them, and
// none of them fires on such a net.
#pragma once

namespace {

int convgForward(hl_learner* h, const ConvArgs& ca, int l, hipStream_t s) {
  char nm[32];
  snprintf(nm, sizeof(nm), "convg_fwd%d", l);
  HIPCK(timed(h, nm, s, [&] { return launch_convg_forward(ca, l, h->convMmax, s); }));
  return HL_OK;
}
// D of layer l - 1: the filter slices per residue class from the step's weights, then the classes' correlations
int convgInputGradient(hl_learner* h, const ConvArgs& ca, int l, hipStream_t s) {
  char nm[32];
  snprintf(nm, sizeof(nm), "convg_prep%d", l);
  HIPCK(timed(h, nm, s, [&] { return launch_convg_prep(ca, l, s); }));
  snprintf(nm, sizeof(nm), "convg_dx%d", l);
  HIPCK(timed(h, nm, s, [&] { return launch_convg_dx(ca, l, s); }));
  return HL_OK;
}
// the partial filter gradients of every such layer (joined, with conv.hip's, by conv_reduce_adam_kernel)
int convgFilterGradients(hl_learner* h, const ConvArgs& ca, hipStream_t s) {
  char nm[32];
  for (int l = 0; l < h->nConv; ++l) if (ca.L[l].gen) {
    snprintf(nm, sizeof(nm), "convg_dw%d", l);
    HIPCK(timed(h, nm, s, [&] { return launch_convg_dw(ca, l, s); }));
  }
  return HL_OK;
}

}  // namespace
