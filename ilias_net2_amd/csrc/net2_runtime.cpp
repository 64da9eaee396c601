/*
 * net2_runtime.cpp -- the runtime and device layer under the C ABI: HIP
 * errors and fault injection, devices and the thread's selection, NUMA
 * placement, page-lock lookups, the per-device context and its slots'
 * lifecycle, and the small exported calls that belong to them.
 */
#include "net2_host.h"
#include "sha2_coalesce.h"

thread_local int tl_last_hip_error = 0;

int hip_fail(hipError_t e)
{
	tl_last_hip_error = (int)e;
	return e == hipErrorOutOfMemory ? ENOMEM : EIO;
}

#if NET2_FAULT_INJECT
namespace {
std::atomic<int> g_fi_site{0}, g_fi_left{0};
}
bool fi_hit(int site)
{
	if (g_fi_site.load(std::memory_order_relaxed) != site)
		return false;
	if (g_fi_left.fetch_sub(1, std::memory_order_relaxed) != 1)
		return false;
	g_fi_site.store(0, std::memory_order_relaxed);
	return true;
}
#endif

/*
 * After a chunk failed part-way: wait for whatever it already queued on its
 * stream (a copy still reading the caller's input or the slot's staging, a
 * kernel still storing into the caller's mapped output), so nothing of the
 * failed call runs after it returns and the slot can be reused.  The first
 * error's HIP code is kept for net2_sha2_last_hip_error.
 */
void quiesce(hipStream_t st)
{
	if (st == nullptr)
		return;
	const int keep = tl_last_hip_error;
	(void)hipStreamSynchronize(st);
	(void)hipGetLastError();
	tl_last_hip_error = keep;
}

bool dbg_timing()
{
	static const bool on = getenv("NET2_SHA2_DEBUG_TIMING") != nullptr;
	return on;
}

/* ---- the pipeline slot and the per-device context ------------------------ */

int Slot::open(size_t *in, size_t *n, bool *fits)
{
	if (stream == nullptr) {
		HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
	}
	*fits = *in <= cap_in && *n <= cap_n;
	/* grow both dimensions monotonically, with headroom: chunks of a
	 * variable-length batch differ slightly in bytes and packet count,
	 * and re-sizing to each one exactly re-allocated the pinned
	 * buffers (~10 ms) on every other chunk */
	*in = std::max<size_t>({*in + *in / 8, cap_in, 4096});
	*n = std::max<size_t>({*n + *n / 4, cap_n, 64});
	return 0;
}

int Slot::grown(void *bin_ws, size_t in, size_t n)
{
	HIP_TRY(net2_bin_ws_init((uint32_t *)bin_ws, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	cap_in = in;
	cap_n = n;
	return 0;
}

int Slot::drain()
{
	if (!busy)
		return 0;
	busy = false;
	std::function<int()> f;
	f.swap(finish);		/* a chunk whose wait fails hands nothing over */
	const double t0 = dbg_now();
	HIP_TRY(hipEventSynchronize(done));
	const double t1 = dbg_now();
	const int rc = f ? f() : 0;
	if (dbg_timing())
		fprintf(stderr, "net2: slot wait %.3f ms, finish %.3f ms\n",
		    t1 - t0, dbg_now() - t1);
	return rc;
}

DeviceCtx *ctx_for(size_t idx)
{
	static std::mutex mu;
	static std::vector<std::unique_ptr<DeviceCtx>> ctx;
	std::lock_guard<std::mutex> g(mu);
	if (ctx.size() <= idx)
		ctx.resize(idx + 1);
	if (!ctx[idx])
		ctx[idx].reset(new DeviceCtx());
	return ctx[idx].get();
}

/* ---- device discovery --------------------------------------------------- */

/* HIP ordinals of the usable gfx950 devices, looked up once. */
const std::vector<int> &devices()
{
	static const std::vector<int> found = []() {
		std::vector<int> v;
		int n = 0;
		if (hipGetDeviceCount(&n) != hipSuccess)
			return v;
		for (int d = 0; d < n; d++) {
			hipDeviceProp_t p;
			if (hipGetDeviceProperties(&p, d) == hipSuccess &&
			    strncmp(p.gcnArchName, "gfx950", 6) == 0)
				v.push_back(d);
		}
		return v;
	}();
	return found;
}

/*
 * Devices a host-memory batch (net2_sha2_batch) is sharded over.  Test
 * knob NET2_SHA2_VIRTUAL_DEVICES=k (read per call): every real device is
 * listed k times, so each entry gets its own DeviceCtx, stream pair and
 * host thread and the multi-device slicing runs on a one-GPU machine.
 */
std::vector<int> batch_devices()
{
	std::vector<int> dv = devices();
	const char *v = getenv("NET2_SHA2_VIRTUAL_DEVICES");
	const int k = v != nullptr ? atoi(v) : 1;
	if (k > 1 && k <= 64 && !dv.empty()) {
		const std::vector<int> real = dv;
		for (int r = 1; r < k; r++)
			dv.insert(dv.end(), real.begin(), real.end());
	}
	return dv;
}

/*
 * Least payload per device slice of net2_sha2_batch (NET2_SHA2_SLICE_MIN_BYTES,
 * read per call; default 16 MiB, 0 = no limit).  A small batch's latency is
 * one lane's serial chain of compressions, which more devices do not
 * shorten, while each extra device costs a host thread, its own copies and
 * a synchronisation: a 4096 x 1 KiB signing tick stays on one GPU, a 1 GiB
 * batch spreads over eight.
 */
uint64_t slice_min_bytes()
{
	const char *v = getenv("NET2_SHA2_SLICE_MIN_BYTES");
	if (v == nullptr || *v == '\0')
		return 16ull << 20;
	return strtoull(v, nullptr, 10);
}

/* Is the calling thread's current device one we built code for? */
int check_current_device()
{
	int cur = -1;
	const std::vector<int> &dv = devices();
	if (dv.empty())
		return ENODEV;
	if (hipGetDevice(&cur) != hipSuccess)
		return ENODEV;
	return std::find(dv.begin(), dv.end(), cur) != dv.end() ? 0 : ENODEV;
}

/*
 * The calling thread's device selection (net2_sha2_set_device): an index
 * into the device list (batch_devices()), or -1 to follow the thread's
 * current HIP device.  Helper threads that run work submitted by another
 * thread (the signed carver's pool) take the submitter's selection.
 */
static thread_local int tl_dev_sel = -1;

/* The device (index into dv = batch_devices()) a single-message call runs
 * on: the thread's selection; else its current HIP device when that is a
 * usable one (one process per GPU stays on its GPU); else the first. */
size_t small_device(const std::vector<int> &dv)
{
	if (tl_dev_sel >= 0 && (size_t)tl_dev_sel < dv.size())
		return (size_t)tl_dev_sel;
	int cur = -1;
	(void)hipGetDevice(&cur);
	for (size_t d = 0; d < dv.size(); d++)
		if (dv[d] == cur)
			return d;
	return 0;
}

/*
 * NUMA placement of a device's host-side work.  A host-memory batch is
 * sharded over every GPU, one host thread per device (net2_sha2_batch); the
 * thread packs pageable input into pinned staging, and the staging is
 * allocated (and first touched) by it.  On a two-socket host half of the
 * GPUs hang off the other socket, so an unplaced thread pulls its slice's
 * ~55 GB/s of H2D traffic across the socket link.  The slice thread -- and
 * the pack pool threads it starts, which inherit its mask -- is bound to the
 * CPUs of the device's node (sysfs numa_node of its PCI function, within the
 * process's CPUs) for the slice, and restored after.  NET2_SHA2_NUMA=0
 * turns it off.  Slice 0 runs on the calling thread, so for the duration of
 * a net2_sha2_batch call that thread's affinity is the node's CPUs (its own
 * mask is restored before the call returns; include/net2/sha2_batch.h).
 */
namespace {

bool parse_cpulist(const char *s, cpu_set_t *set)
{
	CPU_ZERO(set);
	while (*s && *s != '\n') {
		char *e;
		long a = strtol(s, &e, 10), b = a;
		if (e == s)
			return false;
		if (*e == '-') {
			s = e + 1;
			b = strtol(s, &e, 10);
			if (e == s)
				return false;
		}
		for (long c = a; c <= b && c < CPU_SETSIZE; c++)
			if (c >= 0)
				CPU_SET((int)c, set);
		s = *e == ',' ? e + 1 : e;
	}
	return true;
}

/*
 * The CPUs this process may run on, whoever asks: the cgroup's effective
 * cpuset when it is readable, else the affinity of the thread that loaded
 * the library.  Not the calling thread's own mask: a caller pinned to one
 * CPU must not narrow the placement every later slice of the device gets
 * (the result is cached per device).
 */
cpu_set_t g_load_mask;
bool g_load_mask_ok = false;

__attribute__((constructor)) void capture_load_mask()
{
	g_load_mask_ok = sched_getaffinity(0, sizeof(g_load_mask),
	    &g_load_mask) == 0;
}

bool process_cpus(cpu_set_t *out)
{
	char buf[4096];
	FILE *f = fopen("/sys/fs/cgroup/cpuset.cpus.effective", "r");
	if (f != nullptr) {
		const bool ok = fgets(buf, sizeof(buf), f) != nullptr &&
		    parse_cpulist(buf, out) && CPU_COUNT(out) > 0;
		fclose(f);
		if (ok)
			return true;
	}
	if (g_load_mask_ok) {
		*out = g_load_mask;
		return true;
	}
	return sched_getaffinity(0, sizeof(*out), out) == 0;
}

}	/* namespace */

const NumaPlace &numa_place(int ordinal)
{
	static std::mutex mu;
	static std::vector<std::unique_ptr<NumaPlace>> cache;
	std::lock_guard<std::mutex> g(mu);
	if (cache.size() <= (size_t)ordinal)
		cache.resize((size_t)ordinal + 1);
	if (cache[ordinal])
		return *cache[ordinal];
	std::unique_ptr<NumaPlace> p(new NumaPlace());
	CPU_ZERO(&p->cpus);
	char bus[64] = { 0 }, path[160], buf[4096];
	if (hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, ordinal) == hipSuccess) {
		for (char *c = bus; *c; c++)
			if (*c >= 'A' && *c <= 'F')
				*c = (char)(*c - 'A' + 'a');
		snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node",
		    bus);
		FILE *f = fopen(path, "r");
		if (f != nullptr) {
			if (fscanf(f, "%d", &p->node) != 1)
				p->node = -1;
			fclose(f);
		}
	} else {
		(void)hipGetLastError();
	}
	if (p->node >= 0) {
		snprintf(path, sizeof(path),
		    "/sys/devices/system/node/node%d/cpulist", p->node);
		FILE *f = fopen(path, "r");
		cpu_set_t node_cpus, mine;
		if (f != nullptr && fgets(buf, sizeof(buf), f) != nullptr &&
		    parse_cpulist(buf, &node_cpus) && process_cpus(&mine)) {
			CPU_AND(&p->cpus, &node_cpus, &mine);
			p->have = CPU_COUNT(&p->cpus) > 0;
		}
		if (f != nullptr)
			fclose(f);
	}
	cache[ordinal] = std::move(p);
	return *cache[ordinal];
}

bool numa_enabled()
{
	const char *e = getenv("NET2_SHA2_NUMA");
	return e == nullptr || strcmp(e, "0") != 0;
}

/* Page-locked (pinned or registered) host memory can be DMA'd directly. */
bool is_pinned(const void *p)
{
	hipPointerAttribute_t a;
	if (p == nullptr || hipPointerGetAttributes(&a, p) != hipSuccess) {
		(void)hipGetLastError();	/* clear the sticky lookup error */
		return false;
	}
	return a.type == hipMemoryTypeHost;
}

/*
 * [p, p + bytes) lies in one page-locked allocation, so the GPU may DMA from
 * it or store into it through its device mapping: both ends are page-locked,
 * map to the device at the same distance as on the host, and belong to the
 * same allocation (the same HIP buffer id).
 * A range that only starts in a registered region -- or spans two adjacent
 * page-locked allocations -- fails, and the caller stages it instead.
 */
bool pinned_span(const void *p, size_t bytes)
{
	if (p == nullptr || bytes == 0)
		return false;
	const uint8_t *a = (const uint8_t *)p, *b = a + bytes - 1;
	hipPointerAttribute_t pa, pb;
	if (hipPointerGetAttributes(&pa, a) != hipSuccess ||
	    hipPointerGetAttributes(&pb, b) != hipSuccess) {
		(void)hipGetLastError();
		return false;
	}
	if (pa.type != hipMemoryTypeHost || pb.type != hipMemoryTypeHost ||
	    pa.devicePointer == nullptr ||
	    (const uint8_t *)pb.devicePointer - (const uint8_t *)pa.devicePointer !=
	    (ptrdiff_t)(bytes - 1))
		return false;
	/* hipMemGetAddressRange reports no base for hipHostRegister'ed memory
	 * on this runtime; the buffer id names the allocation for both kinds
	 * (tools/ptr_probe.py, profiles/round6/ptr_probe.txt) */
	unsigned long long ida = 0, idb = 0;
	if (hipPointerGetAttribute(&ida, HIP_POINTER_ATTRIBUTE_BUFFER_ID,
	    (hipDeviceptr_t)a) != hipSuccess ||
	    hipPointerGetAttribute(&idb, HIP_POINTER_ATTRIBUTE_BUFFER_ID,
	    (hipDeviceptr_t)b) != hipSuccess) {
		(void)hipGetLastError();
		return false;
	}
	return ida == idb && ida != 0;
}

SliceWorker *slice_worker(size_t idx)
{
	static std::mutex mu;
	static std::vector<SliceWorker *> w;	/* never freed, see above */
	std::lock_guard<std::mutex> g(mu);
	if (w.size() <= idx)
		w.resize(idx + 1, nullptr);
	if (w[idx] == nullptr)
		w[idx] = new SliceWorker();
	return w[idx];
}

NET2_EXPORT int net2_coalesce_stats(int device, uint64_t *calls,
    uint64_t *launches)
{
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	if (device < -1 || device >= (int)dv.size())
		return EINVAL;
	net2co::stats(device < 0 ? small_device(dv) : (size_t)device, calls,
	    launches);
	return 0;
}

NET2_EXPORT const int net2_hashmax = kNumRows;

NET2_EXPORT int net2_sha2_abi_version(void)
{
	return NET2_SHA2_ABI_VERSION;
}

NET2_EXPORT int net2_sha2_device_count(int *count)
{
	if (count == nullptr)
		return EINVAL;
	*count = (int)devices().size();
	return *count > 0 ? 0 : ENODEV;
}

NET2_EXPORT int net2_sha2_set_device(int index, int *prev)
{
	if (prev != nullptr)
		*prev = tl_dev_sel;
	if (index == -1) {
		tl_dev_sel = -1;
		return 0;
	}
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	if (index < -1 || index >= (int)dv.size())
		return EINVAL;
	HIP_TRY(hipSetDevice(dv[index]));
	tl_dev_sel = index;
	return 0;
}

NET2_EXPORT int net2_sha2_get_device(int *index)
{
	if (index == nullptr)
		return EINVAL;
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	*index = (int)small_device(dv);
	return 0;
}

#if NET2_FAULT_INJECT
NET2_EXPORT int net2_fault_inject(int site, int k)
{
	if (site < 0 || site > FI_RECORD || k < 0)
		return EINVAL;
	g_fi_site.store(0);
	g_fi_left.store(k);
	g_fi_site.store(k > 0 ? site : 0);
	return 0;
}
#endif

NET2_EXPORT int net2_sha2_last_hip_error(void)
{
	return tl_last_hip_error;
}

NET2_EXPORT const char *net2_sha2_strerror(int err)
{
	switch (err) {
	case 0: return "success";
	case EINVAL: return "invalid argument";
	case ENOMEM: return "out of memory";
	case ENODEV: return "no usable gfx950 (MI355X) device";
	case EIO: return "HIP runtime error";
	case ENOSYS: return "not implemented";
	default: return "unknown error";
	}
}

NET2_EXPORT int net2_sha2_numa_stats(int device, int *numa_node,
    uint64_t *slices, uint64_t *slices_on_node)
{
	const std::vector<int> dv = batch_devices();
	if (dv.empty())
		return ENODEV;
	if (device < 0 || (size_t)device >= dv.size())
		return EINVAL;
	const NumaPlace &np = numa_place(dv[device]);
	DeviceCtx *c = ctx_for((size_t)device);
	if (numa_node)
		*numa_node = np.node;
	if (slices)
		*slices = c->slices.load(std::memory_order_relaxed);
	if (slices_on_node)
		*slices_on_node = c->slices_on_node.load(std::memory_order_relaxed);
	return 0;
}

NET2_EXPORT const char *net2_hash_getname(int alg)
{
	return alg >= 0 && alg < kNumRows ? kRows[alg].name : nullptr;
}

NET2_EXPORT int net2_hash_findname(const char *name)
{
	if (name == nullptr)
		return -1;
	for (int i = 0; i < kNumRows; i++)
		if (strcmp(kRows[i].name, name) == 0)
			return i;
	return -1;
}

NET2_EXPORT int net2_hash_gethashlen(int alg)
{
	return alg >= 0 && alg < kNumRows ? kRows[alg].hashlen : -1;
}

NET2_EXPORT int net2_hash_getkeylen(int alg)
{
	return alg >= 0 && alg < kNumRows ? kRows[alg].keylen : -1;
}
