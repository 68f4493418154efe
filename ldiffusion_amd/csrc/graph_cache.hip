// GraphCache / DeviceBuf: the hipGraph replay cache that the UNet, the nnU-Net head and the instance classifier share (lifecycle: model.h).
#include "model.h"

DeviceBuf::~DeviceBuf() {
  if (p) (void)hipFree(p);
}
void DeviceBuf::ensure(size_t bytes) {
  if (bytes <= cap) return;
  if (p) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipFree(p)); p = nullptr; cap = 0; }   // (a replay enqueued earlier may still use it)
  HIP_CHECK(hipMalloc(&p, bytes));
  cap = bytes;
}

GraphCache::~GraphCache() {
  drop();
  if (cap_stream) (void)hipStreamDestroy(cap_stream);
}
void GraphCache::drop() {
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  exec = nullptr; graph = nullptr; uses = 0;
}
void GraphCache::set_enabled(bool on) {
  if (!on) { HIP_CHECK(hipDeviceSynchronize()); drop(); }   // (a replay of the graph may still be running)
  enabled = on;
}

bool GraphCache::bypass(hipStream_t s) const {
  static const bool env_off = getenv("LDIFF_NO_GRAPH") != nullptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s) (void)hipStreamIsCapturing(s, &cs);   // the legacy default stream cannot be captured
  return !enabled || env_off || prof_enabled() || cs != hipStreamCaptureStatusNone;
}

void GraphCache::run(hipStream_t s, const std::function<Key()>& current_key, std::initializer_list<Staging> staging, const std::function<void()>& eager,
                     const std::function<void(hipStream_t)>& staged, const std::function<void()>& copy_in, const std::function<void()>& copy_out) {
  const Key now = current_key();
  if (now != key) { drop(); key = now; }
  if (uses == 0) {   // first use of this configuration: eager (builds lazily derived weights, sizes the workspaces)
    eager();
    key = current_key();   // the key of what the next use captures: the eager pass may have grown a workspace
    uses = 1;
    return;
  }
  if (uses == 1) {   // second use: capture the same launch sequence on the staging buffers
    for (const Staging& st : staging) st.buf->ensure(st.bytes);
    // capture on a handle-owned stream (the caller's may be the legacy default stream, which cannot be captured); nothing
    // executes during capture, and the instantiated graph is launched on the caller's stream
    if (!cap_stream) HIP_CHECK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
    hipGraph_t g = nullptr;
    try {
      staged(cap_stream);
    } catch (...) {
      (void)hipStreamEndCapture(cap_stream, &g);
      if (g) (void)hipGraphDestroy(g);
      enabled = false;   // this configuration cannot be captured: stay eager (same kernels, same results)
      eager();
      return;
    }
    HIP_CHECK(hipStreamEndCapture(cap_stream, &g));
    graph = g;
    size_t n_nodes = 0;
    if (hipGraphGetNodes(g, nullptr, &n_nodes) == hipSuccess) nodes = (long long)n_nodes;
    HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
    uses = 2;
    ++captures;
  }
  copy_in();
  HIP_CHECK(hipGraphLaunch(exec, s));
  copy_out();
  ++replays;
}
