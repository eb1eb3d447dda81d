// hostjpeg.cpp -- the JPEG source of the host path (hostpath.h): batches of
// coefficient sets whose entropy decode (when still pending), IDCT and colour
// conversion run on the device in front of the resize.  The chunk's layout
// (jpeg_chunk), its staging, the launches, and jpeg_path, the entry point.
#include "hostpath.h"

#include <cstring>

namespace mxd {
namespace capi {

const mxd::jpeg::Coefs* coefs_of(const mxd_jpeg_coefs* c) { return reinterpret_cast<const mxd::jpeg::Coefs*>(c); }

namespace {

int64_t rgb_pitch(int32_t w) { return (((int64_t)w * 3 + 63) & ~(int64_t)63) + 64; }
int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// The image's Huffman tables (consecutive in c.htabs from the index
// returned): a set an earlier image of the chunk already staged is shared
// (files from one encoder carry the same tables: one set per C4 batch instead
// of 128 x ~50 KB staged).
int32_t jpeg_huff_tables(const mxd::jpeg::Coefs* coefs, const mxd::jpeg::EntropyScan& es, JpegChunk& c) {
  std::array<uint64_t, 8> key{};
  for (int t = 0; t < es.ntables; t++)
    key[t] = mxd::jpeg::device_table(coefs, es.table_class[t], es.table_id[t], nullptr);
  for (const auto& ts : c.table_sets)
    if (ts.n == es.ntables && ts.key == key) return ts.first;
  const int32_t at = (int32_t)c.htabs.size();
  c.table_sets.push_back({key, es.ntables, at});
  for (int t = 0; t < es.ntables; t++) {
    c.htabs.emplace_back();
    mxd::jpeg::device_table(coefs, es.table_class[t], es.table_id[t], &c.htabs.back());
    c.huff_search = c.huff_search || c.htabs.back().search != 0;
  }
  return at;
}

// The device entropy decode of one pending image, chunk image k: its image
// record and tables, its segments (their unstuffed bytes placed in the word
// buffer) and its jobs.  Its coefficients go to c.coef_bytes past coef_off.
void jpeg_entropy_jobs(const mxd::jpeg::Coefs* coefs, const mxd::jpeg::CoefInfo& info, int32_t k, JpegChunk& c) {
  const mxd::jpeg::EntropyScan es = mxd::jpeg::entropy_scan(coefs);
  mxd::HuffImgDev h{};
  h.coef = c.coef_bytes / 2;  // coef_off added by jpeg_offsets
  for (int q = 0; q < info.ncomp && q < 4; q++) {
    h.plane[q] = info.comp[q].off;
    h.bw[q] = info.comp[q].bw;
    h.comp_h[q] = (int8_t)info.comp[q].h;
    h.comp_v[q] = (int8_t)info.comp[q].v;
  }
  h.ntables = es.ntables;
  h.bpm = es.bpm;
  h.mcux = es.mcux;
  h.interleaved = es.interleaved;
  h.rst_mcus = es.restart_interval > 0 ? es.restart_interval : (int32_t)std::min<int64_t>(es.mcus, INT32_MAX);
  h.mcus = es.mcus;
  for (int j = 0; j < es.bpm; j++) {
    h.blk_comp[j] = (int8_t)es.blk_comp[j];
    h.blk_dc[j] = (int8_t)es.blk_dc[j];
    h.blk_ac[j] = (int8_t)es.blk_ac[j];
    h.blk_dx[j] = (int8_t)es.blk_dx[j];
    h.blk_dy[j] = (int8_t)es.blk_dy[j];
  }
  h.tables = jpeg_huff_tables(coefs, es, c);
  // subsequence length: kHuffMinBits (MXD_TUNE_HUFF_BITS overrides it;
  // a multiple of 32); segments of any length split over several jobs
  const int32_t knob = g_tune[MXD_TUNE_HUFF_BITS].load();
  const int32_t sub_bits = (int32_t)up(knob > 0 ? knob : kHuffMinBits, 32);
  h.sub_bits = sub_bits;
  c.seg_first[k] = (int32_t)c.raw.size();
  c.seg_count[k] = es.nseg;
  const int32_t img_index = (int32_t)c.himgs.size();
  const int32_t seg_base = (int32_t)c.hsegs.size();
  std::vector<int64_t> sub_first;  // per segment: its first subsequence (image-wide numbering)
  int64_t nsub_img = 0;
  for (int sgi = 0; sgi < es.nseg; sgi++) {
    const int64_t raw = es.seg_end[sgi] - es.seg_begin[sgi];
    mxd::HuffSegDev sd{};
    sd.word = c.words_bytes / 4;
    sd.bits = (int32_t)(8 * es.seg_bytes[sgi]);
    sd.img = img_index;
    sd.mcu0 = (int64_t)sgi * h.rst_mcus;
    sd.mcus = (int32_t)std::min<int64_t>(h.rst_mcus, es.mcus - sd.mcu0);
    sd.nsub = (int32_t)std::max<int64_t>(1, (sd.bits + sub_bits - 1) / sub_bits);
    c.raw.push_back({es.data + es.seg_begin[sgi], es.data + es.seg_end[sgi], c.words_bytes});
    // zero padding past the data: a partial last word's tail and >= 1 zero word,
    // which jpeghuff.hip's LDS reader reads for every word past the segment
    c.words_bytes += up(raw + 4, 16);
    sub_first.push_back(nsub_img);
    nsub_img += sd.nsub;
    c.hsegs.push_back(sd);
  }
  sub_first.push_back(nsub_img);
  // jobs: runs of at most kHuffJobCap own subsequences (jpeghuff.h
  // huff_job_cuts; MXD_TUNE_HUFF_JOB lowers the cap)
  const int32_t job_knob = g_tune[MXD_TUNE_HUFF_JOB].load();
  const int64_t cap = job_knob > 0 ? std::min<int64_t>(job_knob, mxd::kHuffJobCap) : mxd::kHuffJobCap;
  const std::vector<int64_t> cuts = mxd::huff_job_cuts(sub_first, nsub_img, cap);
  for (size_t q = 0; q + 1 < cuts.size(); q++) {
    const int64_t a0 = cuts[q], b0 = cuts[q + 1];
    const int64_t sa = std::upper_bound(sub_first.begin(), sub_first.end(), a0) - sub_first.begin() - 1;
    const int64_t ja = a0 - sub_first[sa];  // the first own subsequence's index in its segment
    const int64_t warm = std::min<int64_t>(mxd::kHuffWarm, ja);
    const int64_t sl = std::upper_bound(sub_first.begin(), sub_first.end(), b0 - 1) - sub_first.begin() - 1;
    const int64_t jl = b0 - 1 - sub_first[sl];  // the last subsequence's index in its segment
    const mxd::HuffSegDev& s0 = c.hsegs[seg_base + sa];
    const mxd::HuffSegDev& s1 = c.hsegs[seg_base + sl];
    mxd::HuffJobDev jb{};
    jb.seg0 = (int32_t)(seg_base + sa);
    jb.nseg = (int32_t)(sl - sa + 1);
    jb.sub0 = (int32_t)(ja - warm);
    jb.nsub = (int32_t)(b0 - a0 + warm);
    jb.warm = (int32_t)warm;
    jb.pred = ja > 0 ? 1 : 0;
    jb.word0 = s0.word + (((int64_t)jb.sub0 * sub_bits / 32) & ~(int64_t)3);
    // words staged: to the last segment's staged end when the job reaches
    // it, else 4 words past its last subsequence (a step reads <= 2 past)
    const int64_t seg_end = s1.word + up(es.seg_end[sl] - es.seg_begin[sl] + 4, 16) / 4;
    const int64_t end = jl == s1.nsub - 1 ? seg_end : std::min(seg_end, s1.word + (jl + 1) * sub_bits / 32 + 4);
    jb.words16 = (int32_t)((end - jb.word0 + 3) / 4);
    const int64_t with = mxd::jpeg_huff_lds_bytes(es.ntables, jb.nseg, 4 * (int64_t)jb.words16);
    jb.lds = with <= mxd::jpeg_huff_lds_budget() && g_tune[MXD_TUNE_HUFF_GLOBAL].load() == 0 ? 1 : 0;
    c.huff_lds = std::max(c.huff_lds, jb.lds ? with : mxd::jpeg_huff_lds_bytes(es.ntables, jb.nseg, 0));
    c.huff_threads = std::max(c.huff_threads, jb.nsub);
    c.hjobs.push_back(jb);
  }
  c.himgs.push_back(h);
  c.coef_bytes += up(info.coef_count * 2, 256);
}

// One image's planes (IDCT) and colour record.  coef_at: the byte offset of
// its coefficients, in the staged input (host-decoded) or, `pending`,
// relative to coef_off (added by jpeg_offsets).  f: its resize footprint.
void jpeg_planes(const mxd::jpeg::CoefInfo& info, int64_t coef_at, bool pending, const std::array<int32_t, 4>& f,
                 JpegChunk& c) {
  mxd::JpegImgDev m{};
  m.ncomp = info.ncomp == 1 ? 1 : 3;
  // 0 YCbCr -> RGB; 1 the components as they are (RGB, CMYK's C M Y);
  // 2 YCCK: YCbCr -> RGB inverted (jdcolor.c ycck_cmyk_convert's C M Y)
  m.rgb = info.color_space == 2 || info.color_space == 3 ? 1 : info.color_space == 4 ? 2 : 0;
  m.width = info.width;
  m.height = info.height;
  m.pitch = (int32_t)rgb_pitch(info.width);
  m.skip = 0;
  for (int k = 0; k < m.ncomp; k++) {
    const mxd::jpeg::CoefPlane& cp = info.comp[k];
    mxd::JpegPlaneDev p{};
    p.coef = (coef_at + cp.off * 2) / 2;
    p.out = c.samples;
    p.first_block = c.nblocks;
    p.bw = cp.bw;
    p.bh = cp.bh;
    p.qtab = (int32_t)c.qtabs.size();
    p.coded = cp.coded ? 1 : 0;
    p.zigzag = pending ? 1 : 0;  // decoded by jpeg_huff: zig-zag order
    // the footprint on this component's sample grid, one sample wider on
    // each side (fancy upsampling reads a neighbour), in whole blocks
    const int hx = info.max_h / cp.h, vx = info.max_v / cp.v;
    p.bx0 = std::max(0, (f[0] / hx - 1) / 8);
    p.bx1 = std::min(cp.bw, (f[1] / hx + 1) / 8 + 1);
    p.by0 = std::max(0, (f[2] / vx - 1) / 8);
    p.by1 = std::min(cp.bh, (f[3] / vx + 1) / 8 + 1);
    c.qtabs.insert(c.qtabs.end(), cp.q, cp.q + 64);
    c.planes.push_back(p);
    m.plane[k] = c.samples;
    m.stride[k] = cp.bw * 8;
    m.dw[k] = cp.dw;
    m.dh[k] = cp.dh;
    m.hx[k] = hx;
    m.vx[k] = vx;
    // jpeg.cpp upsample_row's choice
    const bool h2 = cp.h * 2 == info.max_h, v2 = cp.v * 2 == info.max_v;
    const bool hf = cp.h == info.max_h, vf = cp.v == info.max_v;
    m.mode[k] = hf && vf                ? mxd::kUpFull
                : h2 && vf              ? (cp.dw > 2 ? mxd::kUpH2V1 : mxd::kUpRep)
                : hf && v2              ? mxd::kUpH1V2
                : h2 && v2 && cp.dw > 2 ? mxd::kUpH2V2
                                        : mxd::kUpRep;
    c.samples += up((int64_t)cp.bw * 8 * cp.bh * 8, 256);
    // jpeg_idct's threads: the plane's needed rectangle, padded to a wave
    // (a wave stays in one plane)
    c.nblocks += ((int64_t)std::max(0, p.bx1 - p.bx0) * std::max(0, p.by1 - p.by0) + 63) & ~(int64_t)63;
  }
  m.out = c.mid_bytes;  // relative to rgb_off (added by jpeg_bind)
  c.mid_bytes += up((int64_t)m.pitch * m.height, 256);
  c.max_quad_rows = std::max<int64_t>(c.max_quad_rows, (int64_t)m.height * ((info.width + 7) / 8));
  c.imgs.push_back(m);
}

// Where the chunk's tables sit in the staged input (from tables_at on), the
// device-only regions past them, and the offsets that depend on those.
void jpeg_offsets(int64_t tables_at, JpegChunk& c) {
  c.rgb_off = c.samples;
  c.mid_bytes += c.samples;
  c.words_off = up(tables_at, 256);
  c.htabs_off = up(c.words_off + c.words_bytes, 256);
  c.himgs_off = up(c.htabs_off + (int64_t)(c.htabs.size() * sizeof(mxd::HuffDev)), 256);
  c.hsegs_off = up(c.himgs_off + (int64_t)(c.himgs.size() * sizeof(mxd::HuffImgDev)), 256);
  c.hjobs_off = up(c.hsegs_off + (int64_t)(c.hsegs.size() * sizeof(mxd::HuffSegDev)), 256);
  c.planes_off = up(c.hjobs_off + (int64_t)(c.hjobs.size() * sizeof(mxd::HuffJobDev)), 256);
  c.imgs_off = up(c.planes_off + (int64_t)(c.planes.size() * sizeof(mxd::JpegPlaneDev)), 256);
  c.q_off = up(c.imgs_off + (int64_t)(c.imgs.size() * sizeof(mxd::JpegImgDev)), 256);
  c.ycc.assign(c.imgs.size(), mxd::YccDev{});
  c.ycc_off = up(c.q_off + (int64_t)(c.qtabs.size() * sizeof(uint16_t)), 16);
  c.end = c.ycc_off + (int64_t)(c.ycc.size() * sizeof(mxd::YccDev));
  c.pub_off = up(c.end, 256);
  c.coef_off = up(c.pub_off + (int64_t)(c.hjobs.size() * sizeof(mxd::HuffPubDev)) + (int64_t)sizeof(mxd::HuffCtlDev),
                  256);
  c.dev_end = c.coef_off + c.coef_bytes;
  for (mxd::HuffImgDev& h : c.himgs) h.coef += c.coef_off / 2;
  for (mxd::JpegPlaneDev& p : c.planes)
    if (p.zigzag) p.coef += c.coef_off / 2;  // (the planes of pending images)
}

// Chunk image j's resize source: its RGB frame in dev_mid, or -- 4:2:0 YCbCr
// that a scatter wave kernel takes -- its sample planes, resized with no RGB
// frame (jpeg_color skips the image).  After the destination is bound:
// ycc_plan_ok plans the image as run_batch will.
void jpeg_bind_image(HostCall& c, int32_t j) {
  const int32_t i = c.cur.first + j;
  const mxd_image& im = c.images[i];
  const mxd_jpeg_image& ji = c.jpeg[i];
  const Slot& sl = *c.sl;
  mxd::JpegImgDev& m = c.jc.imgs[j];
  const uint8_t* win = sl.dev_mid + m.out + (int64_t)ji.win_y * m.pitch + (int64_t)ji.win_x * 3;
  c.where[j] = Stored{win, m.pitch, 0, 0, im.src_h};
  c.dev_imgs[j].src = win;
  c.dev_imgs[j].src_stride = m.pitch;
  const bool h2v2 = m.ncomp == 3 && !m.rgb && m.mode[0] == mxd::kUpFull && m.mode[1] == mxd::kUpH2V2 &&
                    m.mode[2] == mxd::kUpH2V2 && m.stride[1] == m.stride[2] && m.dw[1] == m.dw[2] &&
                    m.dh[1] == m.dh[2] && m.plane[0] < m.plane[1] && m.plane[1] < m.plane[2];
  if (!h2v2 || g_tune[MXD_TUNE_JPEG_RGB].load() == 1 || (ji.win_x & 3) != 0) return;
  mxd::YccDev& y = c.jc.ycc[j];
  y.cb = m.plane[1] - m.plane[0];
  y.cr = m.plane[2] - m.plane[0];
  y.ystride = m.stride[0];
  y.cstride = m.stride[1];
  y.dw = m.dw[1];
  y.dh = m.dh[1];
  y.win_x = ji.win_x;
  y.win_y = ji.win_y;
  y.records = (int32_t)std::min<int64_t>(y.cr + (int64_t)y.cstride * y.dh, INT32_MAX);
  const Stored planes{sl.dev_mid + m.plane[0], m.stride[0], 0, 0, im.src_h,
                      reinterpret_cast<const mxd::YccDev*>(sl.dev_in + c.jc.ycc_off) + j};
  if (y.cr + (int64_t)y.cstride * y.dh < INT32_MAX &&
      ycc_plan_ok(c.dev_imgs[j], planes, c.launch_dtype(i), c.device)) {
    c.where[j] = planes;  // (dev_imgs[j] keeps the RGB frame's geometry, which run_batch validates)
    m.skip = 1;
    g_plane_sources.fetch_add(1, std::memory_order_relaxed);
  }
}

#ifdef MXD_HUFF_STAMPS
// diagnostic build: the jobs' phase stamps (jpeghuff.hip) appended to $MXD_HUFF_STAMPS_FILE
int huff_stamps_dump(const JpegChunk& jc, const mxd::HuffPubDev* pub, hipStream_t stream) {
  const char* path = getenv("MXD_HUFF_STAMPS_FILE");
  if (!path) return MXD_OK;
  std::vector<mxd::HuffPubDev> rec(jc.hjobs.size());
  MXD_HIP(hipStreamSynchronize(stream));
  MXD_HIP(hipMemcpy(rec.data(), pub, rec.size() * sizeof(mxd::HuffPubDev), hipMemcpyDeviceToHost));
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (FILE* f = fopen(path, "ab")) {
    const int64_t n = (int64_t)rec.size(), words = mxd::kHuffPubWords - 8;
    fwrite(&n, 8, 1, f);
    fwrite(&words, 8, 1, f);
    for (const auto& r : rec) fwrite(&r.w[8], 8, mxd::kHuffPubWords - 8, f);
    for (const auto& j : jc.hjobs) fwrite(&j, sizeof(j), 1, f);
    fclose(f);
  }
  return MXD_OK;
}
#endif

}  // namespace

void jpeg_chunk(const mxd_jpeg_image* jimg, const Stage* st, ChunkRange r, int64_t tables_at, JpegChunk* out) {
  JpegChunk& c = *out;
  c = JpegChunk();
  c.seg_first.assign(r.end - r.first, -1);
  c.seg_count.assign(r.end - r.first, 0);
  for (int32_t i = r.first; i < r.end; i++) {
    const mxd::jpeg::Coefs* coefs = coefs_of(jimg[i].coefs);
    const mxd::jpeg::CoefInfo info = mxd::jpeg::coef_info(coefs);
    // host-decoded coefficients: staged at in_off; pending: in the device-only region
    const int64_t coef_at = info.entropy_pending ? c.coef_bytes : st[i].in_off;
    if (info.entropy_pending) jpeg_entropy_jobs(coefs, info, i - r.first, c);
    jpeg_planes(info, coef_at, info.entropy_pending, st[i].foot, c);
  }
  jpeg_offsets(tables_at, c);
}

int jpeg_plan_input(HostCall& c, int32_t i) {
  const mxd_image& im = c.images[i];
  const mxd_jpeg_image& ji = c.jpeg[i];
  const mxd::jpeg::CoefInfo info = mxd::jpeg::coef_info(coefs_of(ji.coefs));
  Stage& s = c.st[i];  // (the raw source's fields stay zero)
  s.in_size = info.coef_count * 2;  // chunk sizing (device memory); staged only when decoded on the host
  s.pending = info.entropy_pending;
  // the resize's source footprint in the window, as image pixels (the whole
  // window when the geometry has no tables: run_batch reports that)
  const DevTable *xt = nullptr, *yt = nullptr;
  int32_t xl = 0, xh = im.src_w - 1, yl = 0, yh = im.src_h - 1;
  if (tables().get(c.device, im.src_w, im.resize_w, &xt, im.filter) == MXD_OK &&
      tables().get(c.device, im.src_h, im.resize_h, &yt, im.filter) == MXD_OK)
    footprint(*xt, *yt, im, &xl, &xh, &yl, &yh);
  s.foot = {ji.win_x + xl, ji.win_x + xh, ji.win_y + yl, ji.win_y + yh};
  return MXD_OK;
}

int jpeg_lay_out(HostCall& c) {
  int64_t at = 0;
  for (int32_t i = c.cur.first; i < c.cur.end; i++)
    if (!c.st[i].pending) {
      c.st[i].in_off = at;
      at += (c.st[i].in_size + 255) & ~(int64_t)255;
    }
  jpeg_chunk(c.jpeg, c.st.data(), c.cur, at, &c.jc);
  // coefficients, then the chunk's tables, then the entropy decode's
  // publication records and launch control (zeros), in one copy
  c.in_bytes = c.in_staged = c.jc.hjobs.empty() ? c.jc.end : c.jc.coef_off;
  c.dev_in_bytes = c.jc.dev_end;  // + the device-decoded coefficients
  c.zero_copy = false;            // the decode's inputs are copied to the device, its frames resized from there
  return grow_device(&c.sl->dev_mid, &c.sl->dev_mid_cap, c.jc.mid_bytes);
}

void jpeg_stage(HostCall& c, int32_t i) {
  const JpegChunk& jc = c.jc;
  uint8_t* pin_in = c.sl->pin_in;
  if (!c.st[i].pending) {
    std::memcpy(pin_in + c.st[i].in_off, mxd::jpeg::coef_info(coefs_of(c.jpeg[i].coefs)).coef, c.st[i].in_size);
    return;
  }
  // the image's entropy-coded segments, unstuffed, zero padded (the marker
  // parse counted the bytes: HuffSegDev::bits; removing the stuffing on the
  // device instead measured slower)
  const int32_t f = jc.seg_first[i - c.cur.first];
  for (int32_t q = f; q < f + jc.seg_count[i - c.cur.first]; q++) {
    const JpegChunk::Raw& r = jc.raw[q];
    uint8_t* to = pin_in + jc.words_off + r.at;
    const int64_t n = mxd::jpeg::unstuff(r.b, r.e, to);
    std::memset(to + n, 0, (size_t)(((r.e - r.b + 4 + 15) & ~(int64_t)15) - n));
  }
}

int jpeg_bind(HostCall& c) {
  JpegChunk& jc = c.jc;
  Slot& sl = *c.sl;
  for (auto& m : jc.imgs) m.out += jc.rgb_off;
  for (int32_t j = 0; j < c.cur.end - c.cur.first; j++) jpeg_bind_image(c, j);
  // the chunk's tables (after the plane-source decisions: JpegImgDev::skip, ycc)
  auto put = [&](int64_t off, const auto& v) { std::memcpy(sl.pin_in + off, v.data(), v.size() * sizeof(v[0])); };
  put(jc.planes_off, jc.planes);
  put(jc.q_off, jc.qtabs);
  put(jc.imgs_off, jc.imgs);
  put(jc.ycc_off, jc.ycc);
  if (jc.hjobs.empty()) return MXD_OK;
  put(jc.htabs_off, jc.htabs);
  put(jc.himgs_off, jc.himgs);
  put(jc.hsegs_off, jc.hsegs);
  put(jc.hjobs_off, jc.hjobs);
  // the entropy decode's publication records and launch control, staged
  // zero (one copy with the rest instead of a fill), the error word's
  // page-locked host twin in the control record
  if (!sl.huff_err) MXD_HIP(hipHostMalloc(reinterpret_cast<void**>(&sl.huff_err), 64, hipHostMallocDefault));
  // cleared for every staged chunk: a call that left early (another
  // chunk's error, a failed launch) never read the word back, and a job
  // that gave up there must not fail this call
  *sl.huff_err = 0;
  std::memset(sl.pin_in + jc.pub_off, 0, (size_t)(jc.coef_off - jc.pub_off));
  mxd::HuffCtlDev ctl{};
  ctl.err_host = const_cast<int32_t*>(reinterpret_cast<const int32_t*>(host_device_ptr(sl.huff_err)));
  std::memcpy(sl.pin_in + jc.pub_off + jc.hjobs.size() * sizeof(mxd::HuffPubDev), &ctl, sizeof ctl);
  return MXD_OK;
}

int jpeg_enqueue(HostCall& c) {
  const JpegChunk& jc = c.jc;
  const Slot& sl = *c.sl;
  if (!jc.hjobs.empty()) {
    // jpeg_chunk's job sizing keeps every job within one workgroup; a
    // larger one would leave subsequences undecoded and never publish
    if (jc.huff_threads > mxd::kHuffThreads)
      return fail(MXD_ERR_DEVICE, "jpeg entropy decode: a job of " + std::to_string(jc.huff_threads) +
                                      " subsequences exceeds a workgroup");
    // (the publication records and the ticket came zero with the staged
    // copy; the decode zeroes every block it starts, and the blocks
    // insufficient data leaves undecoded)
    auto* pub = reinterpret_cast<mxd::HuffPubDev*>(sl.dev_in + jc.pub_off);
    auto* ctl = reinterpret_cast<mxd::HuffCtlDev*>(pub + jc.hjobs.size());
    if (mxd::launch_jpeg_huff(reinterpret_cast<const uint32_t*>(sl.dev_in + jc.words_off),
                              reinterpret_cast<const mxd::HuffDev*>(sl.dev_in + jc.htabs_off),
                              reinterpret_cast<const mxd::HuffImgDev*>(sl.dev_in + jc.himgs_off),
                              reinterpret_cast<const mxd::HuffSegDev*>(sl.dev_in + jc.hsegs_off),
                              reinterpret_cast<const mxd::HuffJobDev*>(sl.dev_in + jc.hjobs_off),
                              (int32_t)jc.hjobs.size(), jc.huff_threads, jc.huff_lds, pub, ctl,
                              reinterpret_cast<int16_t*>(sl.dev_in), jc.huff_search, sl.stream))
      return fail(MXD_ERR_DEVICE, std::string("jpeg entropy decode launch: ") + hipGetErrorString(hipGetLastError()));
    // (a job that gives up sets *sl.huff_err itself: no copy back)
#ifdef MXD_HUFF_STAMPS
    if (int rc = huff_stamps_dump(jc, pub, sl.stream)) return rc;
#endif
  }
  mxd::launch_jpeg_idct(reinterpret_cast<const int16_t*>(sl.dev_in),
                        reinterpret_cast<const uint16_t*>(sl.dev_in + jc.q_off),
                        reinterpret_cast<const mxd::JpegPlaneDev*>(sl.dev_in + jc.planes_off),
                        (int32_t)jc.planes.size(), jc.nblocks, sl.dev_mid, sl.stream);
  bool rgb_frames = false;  // some image still needs its RGB frame
  for (const auto& m : jc.imgs) rgb_frames = rgb_frames || !m.skip;
  if (rgb_frames)
    mxd::launch_jpeg_color(sl.dev_mid, reinterpret_cast<const mxd::JpegImgDev*>(sl.dev_in + jc.imgs_off),
                           c.cur.end - c.cur.first, jc.max_quad_rows, sl.dev_mid, sl.stream);
  MXD_HIP(hipGetLastError());
  return MXD_OK;
}

int jpeg_path(const mxd_jpeg_image* jimg, int32_t n, int32_t out_dtype, int32_t device, bool dst_device,
              PostOps ops) {
  if (n < 0 || (n > 0 && !jimg)) return fail(MXD_ERR_INVALID, "mxd: bad image array");
  std::vector<mxd_image> imgs(n);
  for (int32_t i = 0; i < n; i++) {
    const mxd_jpeg_image& j = jimg[i];
    const std::string at = " (image " + std::to_string(i) + ")";
    if (!j.coefs) return fail(MXD_ERR_INVALID, "mxd: null coefs" + at);
    const mxd::jpeg::CoefInfo info = mxd::jpeg::coef_info(coefs_of(j.coefs));
    if (!info.device_ok)
      return fail(MXD_ERR_UNSUPPORTED, "mxd: this JPEG finishes on the host (mxd_jpeg_coefs_finish)" + at);
    if (j.win_w <= 0 || j.win_h <= 0)
      return fail(MXD_ERR_INVALID, "image: cannot create image with 0 or negative dimension" + at);
    if (j.win_x < 0 || j.win_y < 0 || (int64_t)j.win_x + j.win_w > info.width ||
        (int64_t)j.win_y + j.win_h > info.height)
      return fail(MXD_ERR_INVALID, "mxd: source window outside the image" + at);
    mxd_image& m = imgs[i];
    m.src = reinterpret_cast<const uint8_t*>(j.coefs);  // validated, never read: host_path decodes the coefficients
    m.src_stride = (int64_t)j.win_w * 3;
    m.src_w = j.win_w;
    m.src_h = j.win_h;
    m.channels = 3;
    m.resize_w = j.resize_w;
    m.resize_h = j.resize_h;
    m.crop_x = j.crop_x;
    m.crop_y = j.crop_y;
    m.crop_w = j.crop_w;
    m.crop_h = j.crop_h;
    m.flip = j.flip;
    m.filter = j.filter;
    m.dst = j.dst;
    m.dst_stride = j.dst_stride;
  }
  return host_path(imgs.data(), n, out_dtype, device, dst_device, jimg, ops);
}

}  // namespace capi
}  // namespace mxd
