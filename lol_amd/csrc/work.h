// lol_amd/csrc/work.h — the regions of one call's work buffer, stated once: over a null base a Work
// only measures (the *_work_len entries), over the caller's buffer it hands out the same regions.  It rounds nothing:
// even() stays with the layouts that round.  Needs no HIP header.
#pragma once
#include <cstdint>

namespace lolhip {

class Work {
 public:
  explicit Work(int64_t* base) : base_(base) {}
  int64_t* take(int64_t words) {                                   // the next region (null when measuring)
    int64_t* p = base_ ? base_ + at_ : nullptr;
    at_ += words;
    if (at_ > top_) top_ = at_;
    return p;
  }
  double* take_f64(int64_t words) { return reinterpret_cast<double*>(take(words)); }
  // alternatives that share storage start at one mark; len() is the high-water mark
  int64_t mark() const { return at_; }
  void rewind(int64_t m) { at_ = m; }
  int64_t len() const { return top_; }

 private:
  int64_t* base_;
  int64_t at_ = 0, top_ = 0;
};

// the words layout(w, args...) takes: what a *_work_len entry returns, and the size of a region that holds a layout whole
template <class F, class... A>
int64_t measure(F layout, const A&... args) {
  Work w(nullptr);
  layout(w, args...);
  return w.len();
}

}  // namespace lolhip
