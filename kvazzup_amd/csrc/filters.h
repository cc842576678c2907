// kvazzup_amd/csrc/filters.h -- Qt-free C++ mirror of the part of uvgComm's filter graph that sits
// on the hot path: the Filter runtime contract (one thread per filter, bounded input deque with the
// HEVC-aware overflow drop, fan-out with deep copies) and the two filters that call the codecs.
//
//   uvgx::Data / VideoInfo / DataType   <- /root/reference/src/media/processing/filter.h:27-92
//   uvgx::Filter                         <- filter.h:97-261, filter.cpp:151-222 (putInput), :297-306 (getInput),
//                                           :364-417 (sendOutput), :425-443 (run), :516-532 (isHEVCIntra/Inter)
//   uvgx::KvazaarFilter                  <- kvazaarfilter.cpp:122-311 (init), :374-450 (feedInput), :453-495
//   uvgx::OpenHEVCFilter                 <- openhevcfilter.cpp:28-74 (init), :103-189 (process), :192-239
//   uvgx::WireAdapter                    <- uvgrtpsender.cpp:104-117 + uvgrtpreceiver.cpp:54-116 (row f2 of
//                                           whole AU out, one NAL with 4-byte start code in)
// The filters talk to the codecs only through include/kvazaar.h and include/openHevcWrapper.h, exactly
// like the reference; QSettings("uvgComm.ini") is replaced by a string map with the same key names
// (src/settingskeys.h:36-67).
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <stdint.h>
#include "../../include/kvazzup_amd.h"
#include "host_pool.h"

namespace uvgx {

enum DataType { DT_NONE = 0, DT_YUV420VIDEO = 1, DT_YUYVVIDEO = (1 << 4), DT_RGB32VIDEO = (1 << 10), DT_HEVCVIDEO = (1 << 14) };      // (filter.h:27-45: the values of the reference's enum)
enum DataSource { DS_UNKNOWN, DS_LOCAL, DS_REMOTE };
enum HEVC_NAL_UNIT_TYPE { TRAIL_R = 1, IDR_W_RADL = 19, VPS_NUT = 32, SPS_NUT = 33, PPS_NUT = 34 };

struct RoiMap { int width = 0, height = 0; std::unique_ptr<int8_t[]> data; };

struct VideoInfo {
  int16_t width = 0, height = 0;
  int32_t framerateNumerator = 0, framerateDenominator = 0;
  bool flippedVertically = false, flippedHorizontally = false;
  RoiMap roi;
};

struct Data {
  DataSource source = DS_UNKNOWN;
  DataType type = DT_NONE;
  std::unique_ptr<uint8_t[]> data;
  uint32_t data_size = 0;
  int64_t creationTimestamp = -1, presentationTimestamp = -1;
  // extension: creationTimestamp at microsecond resolution on the steady clock (the reference's field is whole milliseconds of wall time,
  // filter.cpp initializeData): what the delay statistics below are computed from; travels with the picture through encoder, wire and decoder
  int64_t creationUs = -1;
  std::unique_ptr<VideoInfo> vInfo;
  // extension (not in the reference): picture already resident in HBM (packed I420; with uvgx/inputFormat the packed RGB32 / YUYV picture `type` names); data stays empty
  const void *device_data = nullptr;
  const void *device_planes[3] = {nullptr, nullptr, nullptr}; int device_pitch[3] = {0, 0, 0};   // decoded I420 left in HBM
  // extension (harness only): the payload lies in memory the source keeps alive and unchanged until the picture has left the encoder
  // filter (bench.py's clip) -- what a camera filter would hand over as `data`, without the harness copying it once more
  const uint8_t *host_view = nullptr;
  // extension (harness only; uvgComm never flushes a running graph): no payload -- the encoder filter outputs the pictures it
  // still holds (video/OWF) and the wire adapter sends end-of-sequence NAL units, which drain the decoder's frame threads
  bool flush_marker = false;
};

// delays in microseconds as a histogram: bucket b holds delays in [16 * 2^(b/4), 16 * 2^((b+1)/4)) us -- quarter octaves from 16 us to ~1 s
struct DelayHist {
  static constexpr int kBuckets = 64;
  std::atomic<uint64_t> n[kBuckets] = {}, count{0}, sumUs{0}, maxUs{0};
  void add(int64_t us);
  double percentile(double q) const;                 // upper edge of the bucket that holds the q-quantile (q in 0..1), us
};
// Counterpart of StatisticsInterface (src/statisticsinterface.h:40,52,59): only what the two filters report
struct Stats {
  std::atomic<uint64_t> encodedPackets{0}, encodedBytes{0}, receivedPackets{0}, receivedBytes{0}, droppedPackets{0};
  std::atomic<uint64_t> encodingDelaySumMs{0};
  // what uvgComm shows its user (kvazaarfilter.cpp:478-479 addEncodedPacket's delay; displayfilter.cpp:113-115 totalDelay), here per picture in us:
  // input accepted by the encoder filter -> access unit sent on; -> decoded picture leaving the decoder filter
  DelayHist encodingDelayUs, totalDelayUs;
};

using Settings = std::map<std::string, std::string>;
int64_t now_ms();
int64_t now_us();                                   // steady clock

class Filter {
 public:
  Filter(std::string id, std::string name, Stats *stats, DataType input, DataType output);
  virtual ~Filter();
  virtual bool init() { return true; }
  virtual void updateSettings() {}
  void addOutConnection(Filter *out) { std::lock_guard<std::mutex> l(connectionMutex_); outConnections_.push_back(out); }
  void addDataOutCallback(std::function<void(std::unique_ptr<Data>)> cb) { std::lock_guard<std::mutex> l(connectionMutex_); outDataCallbacks_.push_back(std::move(cb)); }
  void putInput(std::unique_ptr<Data> data);       // any thread
  void start();
  void stop();
  bool isRunning() const { return threadRunning_; }
  DataType inputType() const { return input_; }
  DataType outputType() const { return output_; }
  const std::string &name() const { return name_; }
  uint32_t bufferedInputs();
  bool waitBufferedBelow(uint32_t n, int timeout_ms);     // sleeps until fewer than n inputs are buffered (harness: a paced source)
  uint64_t inputDiscarded() const { return inputDiscarded_; }
  uint64_t busyNs() const { return busyNs_; }             // time spent inside process() (harness statistics)
  double avgQueue() const { return queueSamples_ ? (double)queueSum_ / queueSamples_ : 0.0; }   // inputs buffered, averaged over the arrivals (harness statistics: which filter is the slow one)

 protected:
  virtual void process() = 0;
  std::unique_ptr<Data> getInput();
  void sendOutput(std::unique_ptr<Data> output);
  static Data *deepDataCopy(const Data *original);
  static bool isHEVCIntra(const unsigned char *buff) { return buff[0] == 0 && buff[1] == 0 && buff[2] == 0 && buff[3] == 1 && (buff[4] >> 1) == IDR_W_RADL; }
  static bool isHEVCInter(const unsigned char *buff) { return buff[0] == 0 && buff[1] == 0 && buff[2] == 0 && buff[3] == 1 && (buff[4] >> 1) == TRAIL_R; }
  Stats *getStats() { return stats_; }
  int maxBufferSize_ = 10;                        // -1 = unlimited

 private:
  void run();
  std::string id_, name_;
  Stats *stats_;
  DataType input_, output_;
  std::mutex bufferMutex_, connectionMutex_;
  std::condition_variable hasInput_, inputTaken_cv_;      // inputTaken_cv_: a source pacing itself waits here (waitBufferedBelow)
  std::deque<std::unique_ptr<Data>> inBuffer_;
  std::vector<Filter *> outConnections_;
  std::vector<std::function<void(std::unique_ptr<Data>)>> outDataCallbacks_;
  std::thread thread_;
  std::atomic<bool> running_{false}, threadRunning_{false};
  uint64_t inputTaken_ = 0, inputDiscarded_ = 0, queueSum_ = 0, queueSamples_ = 0;
  std::atomic<uint64_t> busyNs_{0};
};

class KvazaarFilter : public Filter {
 public:
  KvazaarFilter(std::string id, Stats *stats, const Settings *settings);
  ~KvazaarFilter() override;
  bool init() override;
  void updateSettings() override;
  void close();
  kvz_encoder *encoder() { return enc_; }          // tests / bench: profiling hooks of include/kvazzup_amd.h

 protected:
  void process() override;

 private:
  void customParameters();
  void feedInput(std::unique_ptr<Data> input);
  void parseEncodedFrame(kvz_data_chunk *data_out, uint32_t len_out, kvz_picture *recon_pic);
  void sendEncodedFrame(std::unique_ptr<Data> input, std::unique_ptr<uint8_t[]> hevc_frame, uint32_t dataWritten);
  void createInputVector(int size);
  void cleanupInputVector();
  void addInputPic(int index);
  kvz_picture *getNextPic();
  std::string setting(const std::string &key, const std::string &def = "") const;

  const Settings *settings_;
  const kvz_api *api_ = nullptr;
  kvz_config *config_ = nullptr;
  kvz_encoder *enc_ = nullptr;
  int64_t pts_ = 0;
  std::vector<kvz_picture *> inputPics_;
  int nextInputPic_ = -1;
  std::mutex settingsMutex_;
  struct FrameInfo { std::unique_ptr<Data> data; int8_t *roi_array; };
  std::deque<FrameInfo> encodingFrames_;
  // harness setting uvgx/copyThreads (default 4; 1 = the reference's plain memcpy on the filter thread): cores that share the copy
  // of a picture into the kvz_picture
  std::unique_ptr<kvzx::CopyPool> copy_; std::vector<kvzx::CopyPool::Piece> pieces_;
  std::vector<uint8_t> au_;                        // device-input path: access unit buffer
  bool lastInputOnDevice_ = false;
  void drain();
  // harness setting uvgx/inputFormat = rgb32 | rgb32-sse41 | yuyv ("input-format", kvazaar.h): the filter takes DT_RGB32VIDEO / DT_YUYVVIDEO pictures and hands
  // them to the encoder as they are -- where uvgComm's graph puts a conversion filter in front of this one, the encoder's input stage converts on the GPU
  bool packedInput() const { return config_ && config_->input_format != KVZ_INPUT_I420; }
  int encodeRaw(const void *ptr, bool device, uint32_t *n, kvz_frame_info *info);      // the extension entry point for the encoder's format; ptr NULL: the picture in flight
  void sendRaw(uint32_t n);
};

class OpenHEVCFilter : public Filter {
 public:
  OpenHEVCFilter(uint32_t sessionID, Stats *stats, const Settings *settings);
  ~OpenHEVCFilter() override;
  bool init() override;
  void uninit();
  void updateSettings() override;
  OpenHevc_Handle handle() { return handle_; }
  void finishOutput();

 protected:
  void process() override;

 private:
  void sendDecodedOutput(int &gotPicture);
  const Settings *settings_;
  OpenHevc_Handle handle_ = nullptr;
  bool vpsReceived_ = false, spsReceived_ = false, ppsReceived_ = false;
  uint32_t sessionID_;
  int threads_ = -1;
  std::string parallelizationMode_ = "Slice";
  std::deque<std::unique_ptr<Data>> decodingFrames_;
  std::mutex settingsMutex_;
  uint32_t discardedFrames_ = 0;
  bool download_ = true;
  std::unique_ptr<kvzx::CopyPool> copy_; std::vector<kvzx::CopyPool::Piece> pieces_;     // uvgx/copyThreads, as in KvazaarFilter
  // The row copy out of the decoder's frame (openhevcfilter.cpp:212-229) as a stage of its own (uvgx/asyncOutput, default 1): the filter thread
  // hands the frame's description on and goes back to the next NAL unit; pictures leave in order.  The frame's memory stays valid for six
  // further decode calls here (Decoder::kOutRing), not just until the next one as with OpenHEVC, and at most three copies are pending.
  struct OutJob { std::unique_ptr<Data> frame; const uint8_t *y, *u, *v; uint32_t s_stride, qs_stride; int W, H; long call_no = 0; };      // call_no: the decode call that handed the picture out
  void copyOut(OutJob &job);
  void outputStage();
  std::thread outThread_; std::mutex outM_; std::condition_variable outCv_, outSpace_; std::deque<OutJob> outQ_; bool outQuit_ = false, asyncOut_ = true; long decodeCalls_ = 0;
};

// Row f1: the conversion filter the graph inserts after the decoder (yuvtorgb32.cpp:29-64).  Host pictures go through
// kvzx_yuv420_to_rgb32; pictures the decoder left in HBM are converted there into a small ring of device buffers.
class YUVtoRGB32 : public Filter {
 public:
  YUVtoRGB32(std::string id, Stats *stats) : Filter(std::move(id), "YUVtoRGB32", stats, DT_YUV420VIDEO, DT_RGB32VIDEO) {}
  ~YUVtoRGB32() override;
 protected:
  void process() override;
 private:
  static const int kRing = 4;
  void *ring_[kRing] = {nullptr, nullptr, nullptr, nullptr}; size_t ring_bytes_ = 0; int next_ = 0;
};

// Row f2: what uvgRTP does between the two filters in a loop-back: the sender pushes the whole access
// unit (uvgrtpsender.cpp:106), the receiver hands one NAL unit at a time to the decoder, each with a
// 4-byte start code (uvgrtpreceiver.cpp:86-112).
class WireAdapter : public Filter {
 public:
  WireAdapter(std::string id, Stats *stats) : Filter(std::move(id), "WireAdapter", stats, DT_HEVCVIDEO, DT_HEVCVIDEO) { maxBufferSize_ = -1; }
  // harness setting uvgx/wireLossEvery = n > 0: every n-th access unit is lost on the way (never one with parameter sets or an IRAP picture) -- what a UDP path does;
  // the decoder conceals (csrc/decoder.h; harness setting uvgx/concealment = 2 | 3 picks the rule, OpenHEVCFilter::init) and the chain keeps delivering.  lost(): how many went.
  void setLossEvery(int n) { lossEvery_ = n; }
  // harness setting uvgx/wireLossSegmentEvery = n > 0: every n-th VCL NAL unit -- a slice segment, one packet -- is lost, never one of an IRAP picture: what video/Slices is
  // switched on for.  With uvgx/partialPictures = 1 the decoder keeps the rest of the picture (csrc/decoder.h "Partial pictures v1").
  void setLossSegmentEvery(int n) { lossSegmentEvery_ = n; }
  uint64_t lostSegments() const { return lostSegments_.load(); }
  uint64_t lost() const { return lost_.load(); }
 protected:
  void process() override;
 private:
  int lossEvery_ = 0; uint64_t seen_ = 0; std::atomic<uint64_t> lost_{0};
  int lossSegmentEvery_ = 0; uint64_t seenSegments_ = 0; std::atomic<uint64_t> lostSegments_{0};
};

}  // namespace uvgx
