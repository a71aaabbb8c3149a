// Staging of a front-end entry point's arrays (bsgpu_frontend.cpp): the host arrays of one call packed into one device allocation,
// [inputs | outputs | scratch], one copy in, one launch, one copy out.
//
// Two layers.  StageLayout is plain host C++ (no HIP): it places the segments and moves bytes between the caller's arrays and a
// host image, so it runs under the sanitizers as a stand-alone program (tests/plan/test_staging.cpp).  DeviceStage, compiled only
// where the HIP runtime is, owns the allocation and the two copies.
#pragma once
#include <cassert>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bsg {

// What a start table (n + 1 offsets of n items into packed arrays) can get wrong, in the order the entry points report it:
// start[0] != 0, start[k + 1] < start[k], item_ok(k) false, and, once every item passed those, an item longer than max_per_item.
enum StartCheck { kStartOk = 0, kStartNotZero, kStartDecreasing, kStartBadItem, kStartTooLong };
template <class ItemOk> inline StartCheck check_start_table(const int32_t* start, int n, int max_per_item, ItemOk item_ok) {
  if (start[0] != 0) return kStartNotZero;
  for (int k = 0; k < n; ++k) {
    if (start[k + 1] < start[k]) return kStartDecreasing;
    if (!item_ok(k)) return kStartBadItem;
  }
  for (int k = 0; k < n; ++k) if (start[k + 1] - start[k] > max_per_item) return kStartTooLong;
  return kStartOk;
}
inline StartCheck check_start_table(const int32_t* start, int n, int max_per_item = INT_MAX) {
  return check_start_table(start, n, max_per_item, [](int) { return true; });
}

// Segments are declared in order: every in(), then every out(), then every scratch().  Each starts on a 256-byte boundary; a
// zero-byte segment has an offset like any other and its src / dst (which may be null) is never touched.
class StageLayout {
 public:
  static constexpr size_t kAlign = 256;
  int in(const void* src, size_t bytes) { assert(out_end_ == in_end_ && total_ == in_end_); const int id = add(src, nullptr, bytes); in_end_ = out_end_ = total_; return id; }
  // dst null: an optional output the caller did not ask for (the kernel still writes its segment; scatter() skips it)
  int out(void* dst, size_t bytes) { assert(total_ == out_end_); const int id = add(nullptr, dst, bytes); out_end_ = total_; return id; }
  int scratch(size_t bytes) { return add(nullptr, nullptr, bytes); }

  size_t offset(int id) const { return segs_[id].off; }
  size_t in_bytes() const { return in_end_; }                // [0, in_bytes): what goes to the device
  size_t out_bytes() const { return out_end_ - in_end_; }    // [in_bytes, in_bytes + out_bytes): what comes back
  size_t total_bytes() const { return total_; }

  // The host image: the input span after pack(), the output span once the device's has been copied over it.
  unsigned char* image() { return image_.data(); }
  void pack() {
    image_.assign(in_bytes() > out_bytes() ? in_bytes() : out_bytes(), 0);
    for (const Seg& s : segs_) if (s.off < in_end_ && s.bytes) std::memcpy(image_.data() + s.off, s.src, s.bytes);
  }
  void scatter() const {
    for (const Seg& s : segs_) if (s.dst && s.bytes) std::memcpy(s.dst, image_.data() + (s.off - in_end_), s.bytes);
  }
  // an output segment in the host image (the per-item records that the host splits into several caller arrays)
  template <typename T> const T* out_image(int id) const {
    assert(segs_[id].off >= in_end_ && segs_[id].off + segs_[id].bytes <= out_end_);
    return reinterpret_cast<const T*>(image_.data() + (segs_[id].off - in_end_));
  }

 private:
  struct Seg { const void* src; void* dst; size_t bytes, off; };
  int add(const void* src, void* dst, size_t bytes) {
    segs_.push_back(Seg{src, dst, bytes, total_});
    total_ += (bytes + kAlign - 1) / kAlign * kAlign;
    return (int)segs_.size() - 1;
  }
  std::vector<Seg> segs_;
  std::vector<unsigned char> image_;
  size_t in_end_ = 0, out_end_ = 0, total_ = 0;
};

}  // namespace bsg

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace bsg {

// One allocation for a whole layout, freed when the object goes: no exit path of an entry point can leak it.
class DeviceStage {
 public:
  // (the scratch span, and `spare_bytes` behind it, are left uninitialised)
  explicit DeviceStage(StageLayout& layout, size_t spare_bytes = 0) : L_(layout) {
    if (hipMalloc((void**)&d_, L_.total_bytes() + spare_bytes) != hipSuccess) { (void)hipGetLastError(); d_ = nullptr; }   // (clears the sticky error)
  }
  DeviceStage(const DeviceStage&) = delete;
  DeviceStage& operator=(const DeviceStage&) = delete;
  ~DeviceStage() { if (d_) (void)hipFree(d_); }
  explicit operator bool() const { return d_ != nullptr; }   // false: out of device memory
  template <typename T> T* ptr(int id) const { return reinterpret_cast<T*>(d_ + L_.offset(id)); }
  // Packs and sends the inputs, runs `launch` (which enqueues the kernel on `s`), brings the output span back into the host image
  // and waits for the stream.  The first error of the sequence; the stream is waited for in every case.
  template <class Launch> hipError_t run(hipStream_t s, Launch&& launch) {
    L_.pack();
    hipError_t e = hipMemcpyAsync(d_, L_.image(), L_.in_bytes(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) { launch(); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(L_.image(), d_ + L_.in_bytes(), L_.out_bytes(), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    return e != hipSuccess ? e : e2;
  }

 private:
  StageLayout& L_;
  unsigned char* d_ = nullptr;
};

}  // namespace bsg
#endif  // __HIPCC__
