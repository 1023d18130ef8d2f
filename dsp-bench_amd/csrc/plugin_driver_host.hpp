// plugin_driver_host.hpp -- the host's reading of plugin_driver_abi.h, the
// contract with the driver kernels: dspb_render_args / dspb_seg_args (a State
// is bytes here), the round geometry, the counters' slots and the kernel
// lists.  The contract's text has no include guard and takes
// DSPB_LDS_ROUND_BYTES from its includer (hiprtc compiles it as the front of
// kDriver); this header supplies both.  Plain host C++: no HIP.
#pragma once
#include <cstddef>

#ifndef DSPB_LDS_ROUND
#define DSPB_LDS_ROUND (76 * 1024)
#define DSPB_LDS_WGS 2
#endif
// LDS per workgroup round of the LDS-blocks and segment kernels (handed to
// hiprtc as DSPB_LDS_ROUND_BYTES: the round geometry of plugin_driver_abi.h is
// computed from it on both sides), and the persistent grid's workgroups per CU
#define DSPB_LDS_ROUND_BYTES DSPB_LDS_ROUND
constexpr unsigned long long kLdsRoundBytes = DSPB_LDS_ROUND_BYTES;
constexpr unsigned long long kLdsWgPerCu = DSPB_LDS_WGS;

#include "plugin_driver_abi.h"
// the layout of the parent revision's argument blocks, as a host program
// printed it: code objects compiled before the structs were shared still load
static_assert(sizeof(dspb_render_args) == 328 && sizeof(dspb_seg_args) == 448, "argument block sizes");
static_assert(offsetof(dspb_seg_args, R) + offsetof(dspb_render_args, par) == 324, "dspb_render_args.par");
static_assert(offsetof(dspb_seg_args, seg) == 384 && offsetof(dspb_seg_args, perturb) == 424 &&
                  offsetof(dspb_seg_args, split) == 440,
              "dspb_seg_args fields");
