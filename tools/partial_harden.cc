// tools/partial_harden.cc -- a stand-alone hardening run of partial pictures v1 (csrc/decoder.h) on the decoder's HOST half, no Python and no device: a parse-only decoder
// with the option on is fed every stream of a directory (tests/golden/streams) once per VCL NAL unit with that unit left out, then once per pair of adjacent VCL units
// left out.  Every call must return; the run must end clean.  Built with its own main against the host half compiled with -fsanitize=address,undefined
// (make -C kvazzup_amd/csrc harden), so a read or write out of bounds, a leak of a picture taken back, or undefined arithmetic on the new paths ends the run.
//   kvazzup_amd/csrc/build_harden/partial_harden tests/golden/streams
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "openHevcWrapper.h"
#include "kvazzup_amd.h"

static std::vector<uint8_t> slurp(const std::string &path)
{
  std::vector<uint8_t> d;
  if (FILE *fp = fopen(path.c_str(), "rb")) { uint8_t buf[65536]; size_t n; while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) d.insert(d.end(), buf, buf + n); fclose(fp); }
  return d;
}

// one trial: the NAL units but `skip0` and `skip1` (-1: none), then an end of sequence unit; -> calls that returned an error code
static long trial(const std::vector<std::vector<uint8_t>> &nals, int skip0, int skip1, int threads, long *damaged)
{
  OpenHevc_Handle h = libOpenHevcInit(1, 2);
  if (!h || !kvzx_decoder_set_parse_only(h, threads) || !kvzx_decoder_set_partial_pictures(h, 1) || libOpenHevcStartDecoder(h) != 0) { fprintf(stderr, "no decoder\n"); exit(2); }
  long errors = 0;
  for (int k = 0; k < (int)nals.size(); k++)
    if (k != skip0 && k != skip1) errors += libOpenHevcDecode(h, nals[(size_t)k].data(), (int)nals[(size_t)k].size(), k) < 0;
  const uint8_t eos[6] = {0, 0, 0, 1, 36 << 1, 1};
  errors += libOpenHevcDecode(h, eos, 6, 0) < 0;
  *damaged += kvzx_decoder_damage_log(h, nullptr, 0);
  libOpenHevcClose(h);
  return errors;
}

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: %s <directory of .hevc streams>\n", argv[0]); return 2; }
  std::vector<std::string> files;
  if (DIR *d = opendir(argv[1])) { while (dirent *e = readdir(d)) { std::string n = e->d_name; if (n.size() > 5 && n.substr(n.size() - 5) == ".hevc") files.push_back(std::string(argv[1]) + "/" + n); } closedir(d); }
  long trials = 0, errors = 0, damaged = 0;
  for (const std::string &f : files) {
    const std::vector<uint8_t> s = slurp(f);
    std::vector<size_t> at;
    for (size_t i = 0; i + 3 < s.size(); i++) if (!s[i] && !s[i + 1] && !s[i + 2] && s[i + 3] == 1) { at.push_back(i); i += 3; }
    std::vector<std::vector<uint8_t>> nals; std::vector<int> vcl;
    for (size_t k = 0; k < at.size(); k++) {
      const size_t e = k + 1 < at.size() ? at[k + 1] : s.size();
      nals.emplace_back(s.begin() + (long)at[k], s.begin() + (long)e);
      if (e - at[k] > 5 && ((s[at[k] + 4] >> 1) & 63) < 32) vcl.push_back((int)k);
    }
    for (size_t v = 0; v < vcl.size(); v++) { errors += trial(nals, vcl[v], -1, 1 + (int)(v & 3), &damaged); trials++; }
    for (size_t v = 0; v + 1 < vcl.size(); v++) { errors += trial(nals, vcl[v], vcl[v + 1], 1 + (int)(v & 3), &damaged); trials++; }
  }
  printf("partial_harden: %zu streams, %ld trials, %ld calls answered with an error code, %ld runs of missing blocks filed; every call returned\n", files.size(), trials, errors, damaged);
  return files.empty() ? 2 : 0;
}
