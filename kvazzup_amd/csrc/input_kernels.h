// kvazzup_amd/csrc/input_kernels.h -- launchers of input_kernels.hip: the encoder's input stage for packed RGB32 / YUYV pictures ("input-format")
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/kvazaar.h"

namespace kvzx {
size_t input_bytes(int format, int w, int h);      // bytes of one w x h input picture in `format` (enum kvz_input_format)
// packed picture -> the padded planes k_pad_input would write from the converted picture; false: nothing was launched (format, size or alignment)
bool launch_input_packed(int format, const uint8_t *in, int w, int h, uint8_t *dy, uint8_t *du, uint8_t *dv, int cw, int ch, hipStream_t st);
}  // namespace kvzx
