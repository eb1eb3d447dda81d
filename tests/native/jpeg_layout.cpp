// The JPEG chunk layout of the host path (hostjpeg.cpp jpeg_chunk) without a
// device: parses the given files for device entropy, lays out one chunk over
// all of them and prints one FNV-1a fingerprint per table (the records'
// fields, never their padding or a pointer) and every offset / size scalar.
// Built by `make -C mlx-data_amd layout`, run by tests/test_jpeg_layout.py
// against tests/golden/jpeg_chunk_layout.json.
//
//   jpeg_layout FILE[:x0,x1,y0,y1] ...
// The optional suffix is the image's resize footprint (inclusive, image
// pixels; the whole image without it).  MXD_TUNE_HUFF_BITS in the environment
// sets that tuning knob.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "hostpath.h"

namespace {

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  int64_t n = 0;  // values hashed
  void v(int64_t x) {  // every field as 8 little-endian bytes
    for (int k = 0; k < 8; k++) h = (h ^ (uint8_t)((uint64_t)x >> (8 * k))) * 1099511628211ull;
    n++;
  }
  template <class T, size_t N>
  void a(const T (&x)[N]) {
    for (size_t k = 0; k < N; k++) v((int64_t)x[k]);
  }
  void print(const char* name, size_t count) const {
    std::printf("%s %zu %016llx\n", name, count, (unsigned long long)h);
  }
};

}  // namespace

int main(int argc, char** argv) {
  using namespace mxd;
  using namespace mxd::capi;
  if (const char* e = std::getenv("MXD_TUNE_HUFF_BITS")) mxd_set_tuning(MXD_TUNE_HUFF_BITS, std::atoi(e));
  const int32_t n = argc - 1;
  std::vector<std::vector<uint8_t>> files(n);
  std::vector<mxd_jpeg_image> jimg(n);
  std::vector<Stage> st(n);
  int64_t in_bytes = 0;
  for (int32_t i = 0; i < n; i++) {
    std::string arg = argv[i + 1];
    int foot[4] = {-1, 0, 0, 0};
    const size_t colon = arg.rfind(':');
    if (colon != std::string::npos &&
        std::sscanf(arg.c_str() + colon, ":%d,%d,%d,%d", &foot[0], &foot[1], &foot[2], &foot[3]) == 4)
      arg.resize(colon);
    std::ifstream f(arg, std::ios::binary);
    files[i].assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    mxd_jpeg_coefs* coefs = nullptr;
    if (mxd_jpeg_coefs_parse(files[i].data(), files[i].size(), 1, &coefs) != MXD_OK) {
      std::fprintf(stderr, "%s: %s\n", arg.c_str(), mxd_last_error());
      return 1;
    }
    const jpeg::CoefInfo info = jpeg::coef_info(coefs_of(coefs));
    if (!info.device_ok) {
      std::fprintf(stderr, "%s: finishes on the host\n", arg.c_str());
      return 1;
    }
    jimg[i] = mxd_jpeg_image{};
    jimg[i].coefs = coefs;
    Stage& s = st[i];
    s = Stage{};
    s.in_size = info.coef_count * 2;
    s.pending = info.entropy_pending;
    if (foot[0] < 0) s.foot = {0, info.width - 1, 0, info.height - 1};
    else s.foot = {foot[0], foot[1], foot[2], foot[3]};
    // host-decoded coefficients are staged in order, 256-byte aligned
    if (!s.pending) {
      s.in_off = in_bytes;
      in_bytes += (s.in_size + 255) & ~(int64_t)255;
    }
  }
  JpegChunk c;
  jpeg_chunk(jimg.data(), st.data(), ChunkRange{0, n}, in_bytes, &c);

  Fnv h;
  for (const HuffImgDev& x : c.himgs) {
    h.v(x.coef), h.a(x.plane), h.a(x.bw), h.v(x.tables), h.v(x.ntables), h.v(x.bpm), h.v(x.mcux);
    h.v(x.interleaved), h.v(x.rst_mcus), h.v(x.sub_bits), h.v(x.mcus);
    h.a(x.blk_comp), h.a(x.blk_dc), h.a(x.blk_ac), h.a(x.blk_dx), h.a(x.blk_dy), h.a(x.comp_h), h.a(x.comp_v);
  }
  h.print("himgs", c.himgs.size());
  h = Fnv();
  for (const HuffSegDev& x : c.hsegs) h.v(x.word), h.v(x.bits), h.v(x.img), h.v(x.mcu0), h.v(x.mcus), h.v(x.nsub);
  h.print("hsegs", c.hsegs.size());
  h = Fnv();
  for (const HuffJobDev& x : c.hjobs)
    h.v(x.word0), h.v(x.seg0), h.v(x.nseg), h.v(x.sub0), h.v(x.nsub), h.v(x.warm), h.v(x.words16), h.v(x.lds),
        h.v(x.pred);
  h.print("hjobs", c.hjobs.size());
  h = Fnv();
  for (const JpegPlaneDev& x : c.planes)
    h.v(x.coef), h.v(x.out), h.v(x.first_block), h.v(x.bw), h.v(x.bh), h.v(x.qtab), h.v(x.coded), h.v(x.zigzag),
        h.v(x.bx0), h.v(x.bx1), h.v(x.by0), h.v(x.by1);
  h.print("planes", c.planes.size());
  h = Fnv();
  for (const JpegImgDev& x : c.imgs) {
    h.a(x.plane), h.v(x.out), h.a(x.stride), h.a(x.dw), h.a(x.dh), h.a(x.mode), h.a(x.hx), h.a(x.vx);
    h.v(x.ncomp), h.v(x.rgb), h.v(x.width), h.v(x.height), h.v(x.pitch), h.v(x.skip);
  }
  h.print("imgs", c.imgs.size());
  h = Fnv();
  for (const HuffDev& x : c.htabs) {
    h.a(x.step), h.a(x.step_long), h.v(x.long_base), h.v(x.search), h.a(x.maxcode), h.a(x.valoffset), h.a(x.vals);
  }
  h.print("htabs", c.htabs.size());
  h = Fnv();
  for (uint16_t q : c.qtabs) h.v(q);
  h.print("qtabs", c.qtabs.size());
  h = Fnv();
  for (const JpegChunk::Raw& r : c.raw) h.v(r.e - r.b), h.v(r.at);
  h.print("raw", c.raw.size());
  h = Fnv();
  for (int32_t i = 0; i < n; i++) h.v(c.seg_first[i]), h.v(c.seg_count[i]);
  h.print("segs_of_image", (size_t)n);
  h = Fnv();
  for (const JpegChunk::TableSet& t : c.table_sets) h.v(t.n), h.v(t.first);
  h.print("table_sets", c.table_sets.size());
  const std::pair<const char*, int64_t> scalars[] = {
      {"planes_off", c.planes_off}, {"imgs_off", c.imgs_off},   {"q_off", c.q_off},
      {"ycc_off", c.ycc_off},       {"end", c.end},             {"samples", c.samples},
      {"rgb_off", c.rgb_off},       {"mid_bytes", c.mid_bytes}, {"nblocks", c.nblocks},
      {"max_quad_rows", c.max_quad_rows}, {"words_off", c.words_off}, {"words_bytes", c.words_bytes},
      {"htabs_off", c.htabs_off},   {"himgs_off", c.himgs_off}, {"hsegs_off", c.hsegs_off},
      {"hjobs_off", c.hjobs_off},   {"coef_off", c.coef_off},   {"dev_end", c.dev_end},
      {"pub_off", c.pub_off},       {"huff_threads", c.huff_threads}, {"huff_lds", c.huff_lds},
      {"huff_search", c.huff_search ? 1 : 0}, {"ycc", (int64_t)c.ycc.size()}};
  for (const auto& s : scalars) std::printf("%s %lld\n", s.first, (long long)s.second);
  for (int32_t i = 0; i < n; i++) mxd_jpeg_coefs_free(const_cast<mxd_jpeg_coefs*>(jimg[i].coefs));
  return 0;
}
