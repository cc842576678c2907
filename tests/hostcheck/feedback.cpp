// tests/hostcheck/feedback.cpp -- host build of loss-feedback's statement functions (hevc_core.h fb_*; "uvgx loss feedback v1") for
// tests/test_loss_feedback_host.py, which holds them to the statement of record tests/fb_model.py.  Built by that test on its own (g++, into pytest's
// temporary directory), as scenecut.cpp is.  The loops over the cells are what fb_kernels.hip's kernels do with one workgroup.  Test infrastructure.
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../kvazzup_amd/csrc/hevc_core.h"

using namespace kvzx;

extern "C" {

// map |= the cells of the coding tree blocks [first, first + count), dilated where dilate
void hf_seed(uint8_t *map, int cw, int ch, int first, int count, int dilate)
{
  const int gw = cw / 8, gh = ch / 8;
  std::vector<uint8_t> tmp((size_t)gw * gh);
  for (int i = 0; i < gw * gh; i++) tmp[i] = fb_seed_cell(cw, i % gw, i / gw, first, count) ? 1 : 0;
  for (int i = 0; i < gw * gh; i++) if (dilate ? fb_dilated(tmp.data(), gw, gh, i % gw, i / gw) : tmp[i] != 0) map[i] = 1;
}

// map: D of the picture before -> D of the picture whose record (mv [cell][2], info [cell]) is given
void hf_step(uint8_t *map, int cw, int ch, const int16_t *mv, const uint8_t *info, int dilate)
{
  const int gw = cw / 8, gh = ch / 8, n = gw * gh;
  std::vector<uint8_t> tmp((size_t)n);
  for (int i = 0; i < n; i++) tmp[i] = (!(info[i] & (KVZ_FB_CLEAN | 1)) && fb_inter_cell(map, cw, ch, i % gw, i / gw, mv[2 * i], mv[2 * i + 1])) ? 1 : 0;
  for (bool changed = true; changed;) {
    changed = false;
    for (int i = 0; i < n; i++)
      if ((info[i] & 1) && !(info[i] & KVZ_FB_CLEAN) && !tmp[i] && fb_intra_cell(tmp.data(), cw, ch, i % gw, i / gw, (info[i] >> 1) & 7)) { tmp[i] = 1; changed = true; }
  }
  for (int i = 0; i < n; i++) map[i] = (dilate ? fb_dilated(tmp.data(), gw, gh, i % gw, i / gw) : tmp[i] != 0) ? 1 : 0;
}

void hf_info(const uint8_t *intra, const uint8_t *log2, int n, int clean, uint8_t *info) { for (int i = 0; i < n; i++) info[i] = clean ? KVZ_FB_CLEAN : fb_info(intra[i], log2[i]); }

void hf_blocks(const uint8_t *map, int cw, int ch, int me_range, uint8_t *out)
{
  for (int by = 0; by < ch / 32; by++) for (int bx = 0; bx < cw / 32; bx++) fb_block_record(map, cw / 8, ch / 8, bx, by, me_range, out + 2 * (by * (cw / 32) + bx));
}

int hf_reach(int code) { return fb_reach((uint8_t)code); }

}
