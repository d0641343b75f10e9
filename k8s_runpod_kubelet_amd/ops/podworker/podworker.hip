// podworker — the synthetic GPU pod workload used by tests and bench.py, and
// the process the runtime starts for a pod that has no image command.
//
// Stands in for the container image the reference's integration test deploys
// (reference pkg/virtual_kubelet/runpod_test.go:99 runs a CUDA image with
// `nvidia-smi -L`): it opens the ROCr runtime on its *bound* GPUs (the
// binder scopes visibility via ROCR_VISIBLE_DEVICES), verifies the visible
// device count matches the pod's amd.com/gpu request, runs two tiny gfx950
// kernels to prove real GPU access, optionally binds TCP listen ports (for the
// port-readiness gate), then signals readiness by writing "READY\n" to the
// AMDVK_READY_FD pipe inherited from the native launcher, and finally holds
// until SIGTERM (exit 0) or runs for a fixed duration.
//
// This file is host code only and talks to ROCr (hsa.h) directly: no HIP
// runtime is in the process. A pod that only has to prove it got its GPU needs
// one small AQL queue, a ~6 KB code object, two dispatches and one signal
// wait; HIP's platform/stream layer, its lazy fat-binary path, the copy path
// and the user-space teardown at exit are work the result never uses. The
// kernels (still HIP) live in podworker_kernels.hip; the build embeds their
// code object and the kernarg offsets from its metadata as
// podworker_kernels.inc.
//
// Build (ops/build.py does both steps):
//   hipcc --offload-arch=gfx950 -O2 --cuda-device-only --no-gpu-bundle-output
//         podworker_kernels.hip -o podworker_kernels.co
//   g++ -O2 -x c++ podworker.hip -I$ROCM/include -L$ROCM/lib
//         -lhsa-runtime64 -Wl,-rpath,$ROCM/lib -o podworker

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <arpa/inet.h>
#include <netinet/in.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <time.h>
#include <unistd.h>

#include <string>
#include <vector>

// Generated: kPwCodeObject[], kTouchArgOffsets[], kGatherArgOffsets[].
#include "podworker_kernels.inc"

// Leave without user-space teardown: no hsa_shut_down, no destroys. The
// kernel releases a process's GPU state on exit either way, exactly as it
// does for a pod that is SIGKILLed after its grace period.
[[noreturn]] static void finish(int code) {
  fflush(stdout);
  fflush(stderr);
  _exit(code);
}

static const char* status_text(hsa_status_t st) {
  const char* s = nullptr;
  if (hsa_status_string(st, &s) == HSA_STATUS_SUCCESS && s) return s;
  static char buf[32];
  snprintf(buf, sizeof(buf), "HSA status 0x%x", static_cast<unsigned>(st));
  return buf;
}

#define HSA_CHECK(expr)                                                     \
  do {                                                                      \
    hsa_status_t st_ = (expr);                                              \
    if (st_ != HSA_STATUS_SUCCESS && st_ != HSA_STATUS_INFO_BREAK) {        \
      fprintf(stderr, "podworker: %s failed: %s\n", #expr,                  \
              status_text(st_));                                            \
      finish(11);                                                           \
    }                                                                       \
  } while (0)

static volatile sig_atomic_t g_terminate = 0;
static void on_term(int) { g_terminate = 1; }

static double now_ms() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

struct Timing {
  double runtime_init = 0, queue = 0, load = 0, alloc = 0, dispatch_verify = 0;
};

static volatile int g_queue_error = 0;
static volatile hsa_status_t g_queue_status = HSA_STATUS_SUCCESS;
static void on_queue_error(hsa_status_t st, hsa_queue_t*, void*) {
  fprintf(stderr, "podworker: queue error: %s\n", status_text(st));
  g_queue_status = st;
  g_queue_error = 1;
}

struct Agents {
  std::vector<hsa_agent_t> gpus;
  std::vector<hsa_agent_t> cpus;
};

static hsa_status_t collect_agent(hsa_agent_t agent, void* data) {
  hsa_device_type_t type;
  hsa_status_t st = hsa_agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type);
  if (st != HSA_STATUS_SUCCESS) return st;
  auto* a = static_cast<Agents*>(data);
  if (type == HSA_DEVICE_TYPE_GPU) a->gpus.push_back(agent);
  else if (type == HSA_DEVICE_TYPE_CPU) a->cpus.push_back(agent);
  return HSA_STATUS_SUCCESS;
}

struct PoolQuery {
  bool want_kernarg, want_fine, want_coarse;
  bool found;
  hsa_amd_memory_pool_t pool;
};

static hsa_status_t match_pool(hsa_amd_memory_pool_t pool, void* data) {
  auto* q = static_cast<PoolQuery*>(data);
  hsa_amd_segment_t seg;
  hsa_status_t st = hsa_amd_memory_pool_get_info(
      pool, HSA_AMD_MEMORY_POOL_INFO_SEGMENT, &seg);
  if (st != HSA_STATUS_SUCCESS) return st;
  if (seg != HSA_AMD_SEGMENT_GLOBAL) return HSA_STATUS_SUCCESS;
  bool can_alloc = false;
  st = hsa_amd_memory_pool_get_info(
      pool, HSA_AMD_MEMORY_POOL_INFO_RUNTIME_ALLOC_ALLOWED, &can_alloc);
  if (st != HSA_STATUS_SUCCESS) return st;
  if (!can_alloc) return HSA_STATUS_SUCCESS;
  uint32_t flags = 0;
  st = hsa_amd_memory_pool_get_info(
      pool, HSA_AMD_MEMORY_POOL_INFO_GLOBAL_FLAGS, &flags);
  if (st != HSA_STATUS_SUCCESS) return st;
  if (q->want_kernarg && !(flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_KERNARG_INIT))
    return HSA_STATUS_SUCCESS;
  if (q->want_fine && !(flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_FINE_GRAINED))
    return HSA_STATUS_SUCCESS;
  if (q->want_coarse &&
      !(flags & HSA_AMD_MEMORY_POOL_GLOBAL_FLAG_COARSE_GRAINED))
    return HSA_STATUS_SUCCESS;
  q->pool = pool;
  q->found = true;
  return HSA_STATUS_INFO_BREAK;
}

static bool find_pool(const std::vector<hsa_agent_t>& agents, bool kernarg,
                      bool fine, bool coarse, hsa_amd_memory_pool_t* out) {
  for (hsa_agent_t a : agents) {
    PoolQuery q{kernarg, fine, coarse, false, {}};
    HSA_CHECK(hsa_amd_agent_iterate_memory_pools(a, match_pool, &q));
    if (q.found) {
      *out = q.pool;
      return true;
    }
  }
  return false;
}

static hsa_status_t first_isa(hsa_isa_t isa, void* data) {
  *static_cast<hsa_isa_t*>(data) = isa;
  return HSA_STATUS_INFO_BREAK;
}

struct Kernel {
  uint64_t object = 0;
  uint32_t kernarg_size = 0, group_size = 0, private_size = 0;
};

static Kernel lookup_kernel(hsa_executable_t exec, hsa_agent_t agent,
                            const char* name) {
  hsa_executable_symbol_t sym;
  HSA_CHECK(hsa_executable_get_symbol_by_name(exec, name, &agent, &sym));
  Kernel k;
  HSA_CHECK(hsa_executable_symbol_get_info(
      sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &k.object));
  HSA_CHECK(hsa_executable_symbol_get_info(
      sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE,
      &k.kernarg_size));
  HSA_CHECK(hsa_executable_symbol_get_info(
      sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE,
      &k.group_size));
  HSA_CHECK(hsa_executable_symbol_get_info(
      sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE,
      &k.private_size));
  return k;
}

template <typename T>
static void put_arg(char* kernarg, const Kernel& k, size_t offset, T value) {
  if (offset + sizeof(T) > k.kernarg_size) {
    fprintf(stderr, "podworker: kernarg offset %zu past segment size %u\n",
            offset, k.kernarg_size);
    finish(11);
  }
  memcpy(kernarg + offset, &value, sizeof(T));
}

static const uint32_t kBlock = 256;   // fixed workgroup size of both kernels
static const uint32_t kQueuePackets = 64;
static const unsigned int kPoison = 0xDEADBEEFu;  // even: never equals 2i+1

// Fill every field of a dispatch packet but the header and setup words, which
// publish it and are stored last.
static void fill_dispatch(hsa_kernel_dispatch_packet_t* p, const Kernel& k,
                          uint32_t items, void* kernarg,
                          hsa_signal_t completion) {
  p->workgroup_size_x = kBlock;
  p->workgroup_size_y = 1;
  p->workgroup_size_z = 1;
  p->reserved0 = 0;
  p->grid_size_x = (items + kBlock - 1) / kBlock * kBlock;
  p->grid_size_y = 1;
  p->grid_size_z = 1;
  p->private_segment_size = k.private_size;
  p->group_segment_size = k.group_size;
  p->kernel_object = k.object;
  p->kernarg_address = kernarg;
  p->reserved2 = 0;
  p->completion_signal = completion;
}

static void publish(hsa_kernel_dispatch_packet_t* p, bool barrier) {
  uint16_t header =
      (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) |
      ((barrier ? 1 : 0) << HSA_PACKET_HEADER_BARRIER) |
      (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) |
      (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
  uint16_t setup = 1 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS;
  __atomic_store_n(reinterpret_cast<uint32_t*>(p),
                   header | (static_cast<uint32_t>(setup) << 16),
                   __ATOMIC_RELEASE);
}

// The sample set: every multiple of 4099 in the head window plus the last
// element — or, for --verify-all, every element. The one place it is built:
// the run and --dump-sample-set both call this.
static std::vector<int> sample_set(int n, bool verify_all) {
  std::vector<int> sample;
  if (verify_all) {
    sample.resize(n);
    for (int i = 0; i < n; ++i) sample[i] = i;
  } else {
    const int head = n < (1 << 16) ? n : (1 << 16);
    for (int i = 0; i < head; i += 4099) sample.push_back(i);
    sample.push_back(n - 1);
  }
  return sample;
}

static const size_t kMaxInject = 4;            // --inject-store, at most
static const size_t kMaxDumpSamples = 1 << 17; // --dump-samples, at most

// Tests and measurement only; a pod's run has none of these set.
struct TestHooks {
  std::vector<int> inject;    // --inject-store: out[I] = 1 before the gather
  bool dump_samples = false;  // --dump-samples: print dst before comparing
};

// Touch every visible device: queue + code object + two dispatches + verify.
static int touch_gpus(int expect_gpus, int n, bool verify_all,
                      const TestHooks& hooks, Timing* tm) {
  double t0 = now_ms();
  HSA_CHECK(hsa_init());
  Agents agents;
  HSA_CHECK(hsa_iterate_agents(collect_agent, &agents));
  int count = static_cast<int>(agents.gpus.size());
  if (expect_gpus >= 0 && count != expect_gpus) {
    fprintf(stderr, "podworker: visible GPU count %d != expected %d\n", count,
            expect_gpus);
    return 12;
  }
  uint64_t ticks_per_s = 0;
  HSA_CHECK(hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY,
                                &ticks_per_s));
  hsa_amd_memory_pool_t kernarg_pool{}, host_pool{};
  if (count > 0) {
    if (!find_pool(agents.cpus, true, false, false, &kernarg_pool)) {
      fprintf(stderr, "podworker: kernarg pool lookup failed: none found\n");
      return 11;
    }
    if (!find_pool(agents.cpus, false, true, false, &host_pool)) {
      fprintf(stderr,
              "podworker: fine-grained system pool lookup failed: none found\n");
      return 11;
    }
  }
  tm->runtime_init += now_ms() - t0;

  const std::vector<int> sample = sample_set(n, verify_all);
  const int m = static_cast<int>(sample.size());
  const size_t n_inject = hooks.inject.size();

  for (int dev = 0; dev < count; ++dev) {
    hsa_agent_t gpu = agents.gpus[dev];

    t0 = now_ms();
    hsa_amd_memory_pool_t vram_pool{};
    if (!find_pool({gpu}, false, false, true, &vram_pool)) {
      fprintf(stderr,
              "podworker: device memory pool lookup failed: none on dev %d\n",
              dev);
      return 11;
    }
    tm->runtime_init += now_ms() - t0;

    t0 = now_ms();
    hsa_queue_t* queue = nullptr;
    HSA_CHECK(hsa_queue_create(gpu, kQueuePackets, HSA_QUEUE_TYPE_SINGLE,
                               on_queue_error, nullptr, UINT32_MAX, UINT32_MAX,
                               &queue));
    tm->queue += now_ms() - t0;

    t0 = now_ms();
    hsa_code_object_reader_t reader;
    HSA_CHECK(hsa_code_object_reader_create_from_memory(
        kPwCodeObject, sizeof(kPwCodeObject), &reader));
    hsa_executable_t exec;
    HSA_CHECK(hsa_executable_create_alt(
        HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr,
        &exec));
    HSA_CHECK(hsa_executable_load_agent_code_object(exec, gpu, reader, nullptr,
                                                    nullptr));
    HSA_CHECK(hsa_executable_freeze(exec, nullptr));
    Kernel touch = lookup_kernel(exec, gpu, "touch_kernel.kd");
    Kernel gather = lookup_kernel(exec, gpu, "gather_kernel.kd");
    tm->load += now_ms() - t0;

    t0 = now_ms();
    unsigned int* out = nullptr;   // device memory: proves a VRAM alloc + write
    int* idx = nullptr;            // host-visible
    unsigned int* dst = nullptr;   // host-visible: the witness
    char* kernarg = nullptr;
    HSA_CHECK(hsa_amd_memory_pool_allocate(
        vram_pool, static_cast<size_t>(n) * sizeof(unsigned int), 0,
        reinterpret_cast<void**>(&out)));
    HSA_CHECK(hsa_amd_memory_pool_allocate(
        host_pool, static_cast<size_t>(m) * sizeof(int), 0,
        reinterpret_cast<void**>(&idx)));
    HSA_CHECK(hsa_amd_memory_pool_allocate(
        host_pool, static_cast<size_t>(m) * sizeof(unsigned int), 0,
        reinterpret_cast<void**>(&dst)));
    // one kernarg block for both kernels, each segment 64-byte aligned
    const size_t gather_at = (touch.kernarg_size + 63u) & ~size_t(63);
    // --inject-store: one more touch segment per injection, after the gather's
    const size_t inject_at =
        (gather_at + gather.kernarg_size + 63u) & ~size_t(63);
    const size_t inject_stride = (touch.kernarg_size + 63u) & ~size_t(63);
    const size_t kernarg_bytes =
        n_inject ? inject_at + n_inject * inject_stride
                 : gather_at + gather.kernarg_size;
    HSA_CHECK(hsa_amd_memory_pool_allocate(
        kernarg_pool, kernarg_bytes, 0, reinterpret_cast<void**>(&kernarg)));
    HSA_CHECK(hsa_amd_agents_allow_access(1, &gpu, nullptr, idx));
    HSA_CHECK(hsa_amd_agents_allow_access(1, &gpu, nullptr, dst));
    HSA_CHECK(hsa_amd_agents_allow_access(1, &gpu, nullptr, kernarg));
    hsa_signal_t done;
    HSA_CHECK(hsa_signal_create(1, 0, nullptr, &done));
    tm->alloc += now_ms() - t0;

    t0 = now_ms();
    memcpy(idx, sample.data(), static_cast<size_t>(m) * sizeof(int));
    for (int j = 0; j < m; ++j) dst[j] = kPoison;
    memset(kernarg, 0, kernarg_bytes);
    put_arg(kernarg, touch, kTouchArgOffsets[0], out);
    put_arg(kernarg, touch, kTouchArgOffsets[1], n);
    char* gather_args = kernarg + gather_at;
    put_arg(gather_args, gather, kGatherArgOffsets[0],
            static_cast<const unsigned int*>(out));
    put_arg(gather_args, gather, kGatherArgOffsets[1],
            static_cast<const int*>(idx));
    put_arg(gather_args, gather, kGatherArgOffsets[2], dst);
    put_arg(gather_args, gather, kGatherArgOffsets[3], m);
    for (size_t k = 0; k < n_inject; ++k) {
      // touch_kernel(out + I, 1): its lane 0 stores 2*0+1 into out[I]
      char* args = kernarg + inject_at + k * inject_stride;
      put_arg(args, touch, kTouchArgOffsets[0], out + hooks.inject[k]);
      put_arg(args, touch, kTouchArgOffsets[1], 1);
    }

    // Two packets, one doorbell. Bodies first, each header last with a
    // release store; the gather waits for the touch through its barrier bit.
    // Each --inject-store puts one more touch packet between the two, with
    // the barrier bit, so it runs after the touch and before the gather.
    const uint64_t last = 1 + n_inject;  // the gather's place after `at`
    const uint64_t at = hsa_queue_add_write_index_relaxed(queue, last + 1);
    auto* ring = static_cast<hsa_kernel_dispatch_packet_t*>(queue->base_address);
    const uint32_t mask = queue->size - 1;
    hsa_kernel_dispatch_packet_t* p0 = &ring[at & mask];
    hsa_kernel_dispatch_packet_t* p1 = &ring[(at + last) & mask];
    fill_dispatch(p0, touch, static_cast<uint32_t>(n), kernarg,
                  hsa_signal_t{0});
    for (size_t k = 0; k < n_inject; ++k)
      fill_dispatch(&ring[(at + 1 + k) & mask], touch, 1,
                    kernarg + inject_at + k * inject_stride, hsa_signal_t{0});
    fill_dispatch(p1, gather, static_cast<uint32_t>(m), gather_args, done);
    publish(p0, false);
    for (size_t k = 0; k < n_inject; ++k)
      publish(&ring[(at + 1 + k) & mask], true);
    publish(p1, true);
    hsa_signal_store_screlease(queue->doorbell_signal,
                               static_cast<hsa_signal_value_t>(at + last));

    // Bounded wait: 100 ms slices, 10 s in all, no retry.
    const uint64_t slice = ticks_per_s / 10;
    bool completed = false;
    for (int s = 0; s < 100 && !g_queue_error; ++s) {
      if (hsa_signal_wait_scacquire(done, HSA_SIGNAL_CONDITION_LT, 1, slice,
                                    HSA_WAIT_STATE_BLOCKED) < 1) {
        completed = true;
        break;
      }
    }
    if (g_queue_error) {
      fprintf(stderr, "podworker: kernel dispatch failed: %s\n",
              status_text(g_queue_status));
      return 11;
    }
    if (!completed) {
      fprintf(stderr,
              "podworker: completion signal wait failed: timed out after 10 s\n");
      return 11;
    }

    if (hooks.dump_samples)  // what the gather wrote, never the expectation
      for (int j = 0; j < m; ++j)
        printf("podworker: sample dev %d %d %d 0x%08X\n", dev, j, sample[j],
               dst[j]);
    for (int j = 0; j < m; ++j) {
      const int i = sample[j];
      if (dst[j] != static_cast<unsigned int>(i) * 2u + 1u) {
        if (!verify_all && j == m - 1)
          fprintf(stderr, "podworker: kernel verify failed at tail on dev %d\n",
                  dev);
        else
          fprintf(stderr, "podworker: kernel verify failed at %d on dev %d\n",
                  i, dev);
        return 13;
      }
    }
    tm->dispatch_verify += now_ms() - t0;

    char product[64] = {0};
    HSA_CHECK(hsa_agent_get_info(
        gpu, static_cast<hsa_agent_info_t>(HSA_AMD_AGENT_INFO_PRODUCT_NAME),
        product));
    hsa_isa_t isa{};
    HSA_CHECK(hsa_agent_iterate_isas(gpu, first_isa, &isa));
    uint32_t isa_len = 0;
    HSA_CHECK(hsa_isa_get_info_alt(isa, HSA_ISA_INFO_NAME_LENGTH, &isa_len));
    std::string isa_name(isa_len + 1, '\0');
    HSA_CHECK(hsa_isa_get_info_alt(isa, HSA_ISA_INFO_NAME, &isa_name[0]));
    isa_name.resize(strlen(isa_name.c_str()));
    const char prefix[] = "amdgcn-amd-amdhsa--";
    if (isa_name.compare(0, sizeof(prefix) - 1, prefix) == 0)
      isa_name.erase(0, sizeof(prefix) - 1);
    size_t vram_bytes = 0;
    HSA_CHECK(hsa_amd_memory_pool_get_info(
        vram_pool, HSA_AMD_MEMORY_POOL_INFO_SIZE, &vram_bytes));
    printf("podworker: dev %d %s gcnArch=%s vram=%zuMB ok\n", dev, product,
           isa_name.c_str(), vram_bytes >> 20);
  }
  return 0;
}

static int listen_on(int port) {
  int fd = socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
  if (fd < 0) return -1;
  int one = 1;
  setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
  sockaddr_in addr{};
  addr.sin_family = AF_INET;
  addr.sin_addr.s_addr = htonl(INADDR_ANY);
  addr.sin_port = htons(static_cast<uint16_t>(port));
  if (bind(fd, reinterpret_cast<sockaddr*>(&addr), sizeof(addr)) != 0 ||
      listen(fd, 8) != 0) {
    close(fd);
    return -1;
  }
  return fd;
}

int main(int argc, char** argv) {
  const double t_main = now_ms();
  int expect_gpus = -1;     // -1: skip GPU entirely (CPU pod)
  double run_for = -1.0;    // seconds; -1 with hold=true means until SIGTERM
  bool hold = false;
  int exit_code = 0;
  double startup_delay = 0.0;
  std::vector<int> ports;
  long long touch_elems = 1 << 20;  // tests and measurement only
  bool verify_all = false;          // tests and measurement only
  bool dump_sample_set = false;     // tests and measurement only
  TestHooks hooks;                  // tests and measurement only
  std::vector<long long> inject;    // --inject-store, as given

  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
    if (a == "--expect-gpus") expect_gpus = atoi(next());
    else if (a == "--run-for") run_for = atof(next());
    else if (a == "--hold") hold = true;
    else if (a == "--exit-code") exit_code = atoi(next());
    else if (a == "--startup-delay") startup_delay = atof(next());
    else if (a == "--listen-port") ports.push_back(atoi(next()));
    else if (a == "--touch-elems") touch_elems = atoll(next());
    else if (a == "--verify-all") verify_all = true;
    else if (a == "--dump-sample-set") dump_sample_set = true;
    else if (a == "--dump-samples") hooks.dump_samples = true;
    else if (a == "--inject-store") inject.push_back(atoll(next()));
    else if (a == "--fail") {
      fprintf(stderr, "podworker: simulated failure\n");
      finish(1);
    } else {
      fprintf(stderr, "podworker: unknown arg %s\n", a.c_str());
      finish(2);
    }
  }
  // the grid is rounded up to whole workgroups and indices are ints
  if (touch_elems < 1 || touch_elems > (1ll << 28)) {
    fprintf(stderr, "podworker: --touch-elems must be in 1..%lld\n", 1ll << 28);
    finish(2);
  }
  if (verify_all && touch_elems > (1 << 20)) {
    fprintf(stderr, "podworker: --verify-all takes at most %d elements\n",
            1 << 20);
    finish(2);
  }
  if (inject.size() > kMaxInject) {
    fprintf(stderr, "podworker: --inject-store at most %zu times\n",
            kMaxInject);
    finish(2);
  }
  for (long long at : inject) {
    // element 0 already holds 1, and the store must stay inside the buffer
    if (at < 1 || at >= touch_elems) {
      fprintf(stderr, "podworker: --inject-store must be in 1..%lld\n",
              touch_elems - 1);
      finish(2);
    }
    hooks.inject.push_back(static_cast<int>(at));
  }
  if (dump_sample_set || hooks.dump_samples) {
    const std::vector<int> sample =
        sample_set(static_cast<int>(touch_elems), verify_all);
    if (hooks.dump_samples && sample.size() > kMaxDumpSamples) {
      fprintf(stderr, "podworker: --dump-samples takes at most %zu samples\n",
              kMaxDumpSamples);
      finish(2);
    }
    if (dump_sample_set) {
      printf("podworker: sample-set m=%zu\n", sample.size());
      for (size_t j = 0; j < sample.size(); j += 16) {
        printf("podworker: sample-set");
        for (size_t k = j; k < j + 16 && k < sample.size(); ++k)
          printf(" %d", sample[k]);
        printf("\n");
      }
      finish(0);
    }
  }

  struct sigaction sa{};
  sa.sa_handler = on_term;
  sigaction(SIGTERM, &sa, nullptr);
  sigaction(SIGINT, &sa, nullptr);

  if (startup_delay > 0) usleep(static_cast<useconds_t>(startup_delay * 1e6));

  Timing tm;
  if (expect_gpus >= 0) {
    int rc = touch_gpus(expect_gpus, static_cast<int>(touch_elems), verify_all,
                        hooks, &tm);
    if (rc != 0) finish(rc);
  }

  std::vector<int> listen_fds;
  for (int p : ports) {
    int fd = listen_on(p);
    if (fd < 0) {
      fprintf(stderr, "podworker: listen on %d failed\n", p);
      finish(3);
    }
    listen_fds.push_back(fd);
  }

  const char* timing_env = getenv("AMDVK_PODWORKER_TIMING");
  if (timing_env && strcmp(timing_env, "1") == 0) {
    printf("podworker: timing runtime_init_ms=%.3f queue_ms=%.3f load_ms=%.3f "
           "alloc_ms=%.3f dispatch_verify_ms=%.3f to_ready_ms=%.3f\n",
           tm.runtime_init, tm.queue, tm.load, tm.alloc, tm.dispatch_verify,
           now_ms() - t_main);
  }

  // Readiness: the launcher's pipe (event-driven, replaces the reference's
  // 10 s status poll as the readiness signal path).
  const char* ready_env = getenv("AMDVK_READY_FD");
  if (ready_env) {
    int fd = atoi(ready_env);
    const char msg[] = "READY\n";
    ssize_t w = write(fd, msg, sizeof(msg) - 1);
    (void)w;
    close(fd);
  }
  printf("podworker: ready (gpus=%d ports=%zu)\n", expect_gpus, ports.size());
  fflush(stdout);

  if (hold && run_for < 0) {
    while (!g_terminate) pause();
  } else if (run_for > 0) {
    double remaining = run_for;
    while (remaining > 0 && !g_terminate) {
      double chunk = remaining > 0.1 ? 0.1 : remaining;
      usleep(static_cast<useconds_t>(chunk * 1e6));
      remaining -= chunk;
    }
  }
  for (int fd : listen_fds) close(fd);
  printf("podworker: exiting code=%d\n", exit_code);
  finish(exit_code);
}
