// Host side of every packed weight image (the v3d_*_pack entry points): the bf16 split of the fragment words, the
// eval-mode BatchNorm fold, the host image buffer and the upload into a handle's device block.  None of it is on a timed path.
#pragma once
#include <cmath>
#include <vector>

#include "bf16_split.h"
#include "v3d_common.h"

namespace v3d {

// One lane's eight k values of a split-bf16 fragment -> its four hi and four lo words (two bf16 per word, value 2 q in the
// low half): the [hi, lo][lane][4 words] images of costreg, gemm and propagation
inline void split_bf16x8(const float v[8], unsigned hi_words[4], unsigned lo_words[4]) {
  unsigned hi[8], lo[8];
  for (int e = 0; e < 8; ++e) {
    hi[e] = bf16_rne(v[e]);
    lo[e] = bf16_rne(v[e] - bf16_value(hi[e]));
  }
  for (int q = 0; q < 4; ++q) {
    hi_words[q] = hi[2 * q] | (hi[2 * q + 1] << 16);
    lo_words[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
  }
}

// The same split of one value for the byte-addressed images (backbone blocks, pyramid levels)
inline void split_bf16(float v, unsigned short& hi, unsigned short& lo) {
  const unsigned h = bf16_rne(v);
  hi = (unsigned short)h;
  lo = (unsigned short)bf16_rne(v - bf16_value(h));
}

// Eval-mode BatchNorm behind a convolution, y = (x - mean) / sqrt(var + eps) * gamma + beta (mvsnet.py:22,33), as a
// per-channel scale of the weights and a bias.  The float expressions are part of the contract: the images must not change bits.
struct BnFold {
  std::vector<float> scale, bias;
  BnFold(const float* w, const float* b, const float* m, const float* v, float eps, int channels) : scale(channels), bias(channels) {
    for (int c = 0; c < channels; ++c) {
      scale[c] = w[c] / sqrtf(v[c] + eps);
      bias[c] = b[c] - m[c] * scale[c];
    }
  }
  // conv_w viewed as [n_before][channels][n_after] (Conv: [Co][Ci * taps]; ConvTranspose: [Ci][Co][taps]), every weight times
  // its output channel's scale, rounded to float before anything else touches it
  std::vector<float> weights(const float* conv_w, size_t n_before, size_t n_after) const {
    const size_t nc = scale.size();
    std::vector<float> out(n_before * nc * n_after);
    for (size_t i = 0; i < out.size(); ++i) out[i] = conv_w[i] * scale[i / n_after % nc];
    return out;
  }
};

// Host copy of a handle's device block, in floats; every image starts on a 64-float boundary.  reserve() may move the buffer:
// take pointers afterwards.
struct HostImage {
  std::vector<float> data;
  size_t reserve(size_t nfloat) {
    const size_t o = data.size();
    data.resize(o + (nfloat + 63) / 64 * 64, 0.f);
    return o;
  }
  float* at(size_t ofs) { return data.data() + ofs; }
  unsigned* words(size_t ofs) { return reinterpret_cast<unsigned*>(data.data() + ofs); }
};

// A fresh device block holding `bytes` of `host`; on failure nothing stays allocated and *dev is null
template <class T>
int upload(const void* host, size_t bytes, T** dev, const char* what) {
  hipError_t e = hipMalloc((void**)dev, bytes);
  if (e != hipSuccess) { *dev = nullptr; return fail(V3D_ERR_HIP, "hipMalloc(%s): %s", what, hipGetErrorString(e)); }
  e = hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(*dev); *dev = nullptr; return fail(V3D_ERR_HIP, "hipMemcpy(%s): %s", what, hipGetErrorString(e)); }
  return V3D_OK;
}

// The end of a handle (v3d_*_free), and of a pack function whose upload failed
template <class H>
void release(H* h) {
  if (!h) return;
  if (h->dev) (void)hipFree(h->dev);
  delete h;
}

// Last step of every pack function: upload the image into h->dev and hand the handle out, or release it
template <class H>
int finish_pack(H* h, const void* host, size_t bytes, const char* what, H** out_handle) {
  const int rc = upload(host, bytes, &h->dev, what);
  if (rc != V3D_OK) { release(h); return rc; }
  *out_handle = h;
  return V3D_OK;
}

}  // namespace v3d
