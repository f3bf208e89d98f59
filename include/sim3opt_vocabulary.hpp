// sim3opt_vocabulary.hpp -- header-only C++ helper for the vocabulary tree place recognition descends, forwarding to
// the sim3opt_vocabulary_* entry points of libsim3opt (include/sim3opt.h, "batched vocabulary training").
//
// The reference hands DLoopDetector a DBoW2 vocabulary it loads from a file made elsewhere, by DBoW2 on one thread:
//
//     Surf64Vocabulary voc(k, L);                                                  // kitti_surf.cpp:1231 (the typedef)
//     voc.create(features);                 // std::vector<std::vector<std::vector<float>>>: image, feature, 64 floats
//     voc.save("voc.yml.gz");
//     SurfLoopDetector detector(voc, params);                                      // kittiDetector.h:1549-1564
//
// With this helper the tree is trained on the device from the sequence's own descriptors and handed over as arrays:
//
//     sim3opt_shim::VocabularyTrainer voc(k, L);
//     voc.create(features);                                                        // the same argument
//     voc.save("voc.bin");                                                         // this library's own small format
//     sim3opt_shim::LoopDetectorBatch places;
//     voc.feed(places);                                                            // = places.set_vocabulary(...)
//
// PARITY UNPINNED: the reference tree holds neither DBoW2's source nor a vocabulary file; include/sim3opt.h says what
// is the reference's (FSurf64::distance and meanValue) and what is recalled from upstream.  Parsing DBoW2's .yml.gz
// stays the caller's.  No Eigen, no OpenCV, no DBoW2.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sim3opt.h"
#include "sim3opt_frames.hpp"
#include "sim3opt_place.hpp"

namespace sim3opt_shim {

class VocabularyTrainer {
 public:
  // DBoW2's TemplatedVocabulary(k, L, weighting, scoring): the branching and the depth; the weighting is options().idf
  explicit VocabularyTrainer(int k = 10, int L = 5) : b_(sim3opt_vocabulary_create()) {
    sim3opt_vocabulary_options_default(&opt_);
    opt_.k = k;
    opt_.levels = L;
  }
  ~VocabularyTrainer() { sim3opt_vocabulary_destroy(b_); }
  VocabularyTrainer(const VocabularyTrainer&) = delete;
  VocabularyTrainer& operator=(const VocabularyTrainer&) = delete;

  // read at create()
  sim3opt_vocabulary_options& options() { return opt_; }
  const std::string& last_error() const { return err_; }

  // the tree: empty before create() or load()
  int size() const { return (int)parent_.size(); }  // nodes
  int words() const { return n_words_; }
  bool empty() const { return parent_.empty(); }
  const std::vector<int32_t>& parent() const { return parent_; }
  const std::vector<float>& centre() const { return centre_; }
  const std::vector<double>& weight() const { return weight_; }
  const std::vector<int32_t>& word_id() const { return word_id_; }

  // voc.create(features): features[image][feature] is a descriptor of 64 floats; an image may have none.  The number
  // of nodes, or a negative SIM3OPT_ERR_* with the reason in last_error() and the tree as it was.
  int create(const std::vector<std::vector<std::vector<float>>>& features) {
    std::vector<int32_t> kp_ptr(1, 0);
    std::vector<float> desc;
    for (const auto& image : features) {
      for (const auto& f : image) {
        if (f.size() != 64) return fail("create: a descriptor that is not 64 floats", SIM3OPT_ERR_ARG);
        desc.insert(desc.end(), f.begin(), f.end());
      }
      kp_ptr.push_back((int32_t)(desc.size() / 64));
    }
    return create((int)features.size(), kp_ptr.data(), desc.data());
  }

  // ... and over the arrays of sim3opt_place_batch_set_frames
  int create(int n_frames, const int32_t* kp_ptr, const float* desc) {
    if (!b_) return fail("create: out of memory", SIM3OPT_ERR_ARG);
    const float none = 0.f;  // (the C-ABI refuses a NULL array; images without descriptors still have one)
    int rc = sim3opt_vocabulary_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) rc = sim3opt_vocabulary_set_frames(b_, n_frames, kp_ptr, desc ? desc : &none);
    if (rc == SIM3OPT_OK) rc = sim3opt_vocabulary_train(b_);
    if (rc < 0) return fail(sim3opt_vocabulary_last_error(b_), rc);
    const std::size_t n = (std::size_t)rc;
    parent_.assign(n, 0); centre_.assign(64 * n, 0.f); weight_.assign(n, 0.0); word_id_.assign(n, 0);
    (void)sim3opt_vocabulary_get_vocabulary(b_, parent_.data(), centre_.data(), weight_.data(), word_id_.data());
    count_words();
    return rc;
  }

  // ... and over the frames of a FrameStore, read where they are on the device (sim3opt_vocabulary_set_frames_from)
  int create(FrameStore& store) {
    if (!b_) return fail("create: out of memory", SIM3OPT_ERR_ARG);
    int rc = sim3opt_vocabulary_set_options(b_, &opt_);
    if (rc == SIM3OPT_OK) rc = sim3opt_vocabulary_set_frames_from(b_, store.handle());
    if (rc == SIM3OPT_OK) rc = sim3opt_vocabulary_train(b_);
    if (rc < 0) return fail(sim3opt_vocabulary_last_error(b_), rc);
    const std::size_t n = (std::size_t)rc;
    parent_.assign(n, 0); centre_.assign(64 * n, 0.f); weight_.assign(n, 0.0); word_id_.assign(n, 0);
    (void)sim3opt_vocabulary_get_vocabulary(b_, parent_.data(), centre_.data(), weight_.data(), word_id_.data());
    count_words();
    return rc;
  }

  // The trained (or loaded) tree becomes the detector's vocabulary.  SIM3OPT_OK, SIM3OPT_ERR_STATE without a tree, or
  // what LoopDetectorBatch::set_vocabulary returns.
  int feed(LoopDetectorBatch& detector) {
    if (empty()) return fail("feed: no vocabulary yet", SIM3OPT_ERR_STATE);
    const int rc = detector.set_vocabulary(size(), parent_.data(), centre_.data(), weight_.data(), word_id_.data());
    if (rc != SIM3OPT_OK) return fail(detector.last_error(), rc);
    return rc;
  }

  int save(const std::string& path) {
    if (empty()) return fail("save: no vocabulary yet", SIM3OPT_ERR_STATE);
    const int rc = sim3opt_vocabulary_save(path.c_str(), size(), parent_.data(), centre_.data(), weight_.data(), word_id_.data());
    return rc == SIM3OPT_OK ? rc : fail("save: cannot write " + path, rc);
  }

  int load(const std::string& path) {
    int32_t n = 0, *p = nullptr, *w = nullptr;
    float* c = nullptr;
    double* g = nullptr;
    const int rc = sim3opt_vocabulary_load(path.c_str(), &n, &p, &c, &g, &w);
    if (rc != SIM3OPT_OK) return fail("load: " + path + " is not a readable sim3opt vocabulary file", rc);
    parent_.assign(p, p + n); centre_.assign(c, c + 64 * (std::size_t)n); weight_.assign(g, g + n); word_id_.assign(w, w + n);
    sim3opt_vocabulary_free(p); sim3opt_vocabulary_free(c); sim3opt_vocabulary_free(g); sim3opt_vocabulary_free(w);
    count_words();
    return rc;
  }

 private:
  int fail(const std::string& why, int rc) { err_ = why; return rc; }
  void count_words() {
    n_words_ = 0;
    for (int32_t w : word_id_) n_words_ += w >= 0;
  }

  sim3opt_vocabulary* b_;
  sim3opt_vocabulary_options opt_;
  std::string err_;
  std::vector<int32_t> parent_, word_id_;
  std::vector<float> centre_;
  std::vector<double> weight_;
  int n_words_ = 0;
};

}  // namespace sim3opt_shim
