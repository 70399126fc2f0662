// nrs_mesh.hip — the launches of the mesh sampling (nrs_mesh.h has the owner, nrs_kernels_mesh.h the kernels, nrs_host_mesh.h the
// decisions) and its two context-free entry points, nrs_mesh_field and nrs_mesh_particles: the one translation unit of
// libnereus_hip.so that compiles the kernels.
#include "nrs_mesh.h"

#include "nrs_kernels_mesh.h"

namespace nrs {

static inline uint32_t mesh_blocks(uint64_t n) { return (uint32_t)((n + MESH_BLOCK - 1) / MESH_BLOCK); }

int MeshSampler::upload(const nrs_mesh &mesh, hipStream_t stream)
{
    std::vector<double> tri9;
    mesh_gather(mesh, tri9);
    NRSCHK(tri.alloc(sizeof(double) * tri9.size()));
    HIPCHK(hipMemcpyAsync(tri.p, tri9.data(), sizeof(double) * tri9.size(), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    nt = (uint32_t)mesh.nt;
    return NRS_OK;
}

// the field of the m nodes from `first` on into the batch buffers: the winding number, the distance outputs, or both
int MeshSampler::batch_field(const Lattice &L, uint64_t first, uint32_t m, bool wind, bool dist, hipStream_t stream)
{
    if (wind) NRSCHK(w.alloc(sizeof(double) * (size_t)m));
    if (dist) {
        NRSCHK(d2.alloc(sizeof(double) * (size_t)m));
        NRSCHK(near.alloc(sizeof(uint32_t) * (size_t)m));
        NRSCHK(q.alloc(3 * sizeof(double) * (size_t)m));
    }
    const MeshFieldOut O{w.as<double>(), d2.as<double>(), near.as<uint32_t>(), q.as<double>()};
    const dim3 grid(mesh_blocks(m)), block(MESH_BLOCK);
    const double *T = tri.as<double>();
    if (wind && dist) hipLaunchKernelGGL((k_mesh_field<true, true>), grid, block, 0, stream, L, first, m, T, nt, O);
    else if (wind) hipLaunchKernelGGL((k_mesh_field<true, false>), grid, block, 0, stream, L, first, m, T, nt, O);
    else hipLaunchKernelGGL((k_mesh_field<false, true>), grid, block, 0, stream, L, first, m, T, nt, O);
    HIPCHK(hipGetLastError());
    return NRS_OK;
}

int MeshSampler::field(const Lattice &L, uint64_t nodes, double *winding, double *dist2, uint32_t *nearest, double *closest3, hipStream_t stream)
{
    const bool wind = winding != nullptr, dist = dist2 || nearest || closest3;
    if (!wind && !dist) return NRS_OK;
    for (uint64_t b = 0; b < mesh_batches(nodes); ++b) {
        uint64_t first;
        uint32_t m;
        mesh_batch(nodes, b, first, m);
        NRSCHK(batch_field(L, first, m, wind, dist, stream));
        if (winding) HIPCHK(hipMemcpyAsync(winding + first, w.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream));
        if (dist2) HIPCHK(hipMemcpyAsync(dist2 + first, d2.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream));
        if (nearest) HIPCHK(hipMemcpyAsync(nearest + first, near.p, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        if (closest3) HIPCHK(hipMemcpyAsync(closest3 + 3 * first, q.p, 3 * sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    return NRS_OK;
}

int MeshSampler::select(const Lattice &L, uint64_t nodes, const nrs_mesh_rule &r, uint64_t limit, hipStream_t stream, uint64_t *count)
{
    const MeshSelect S = mesh_select_from(r);
    snapped = (r.flags & NRS_MESH_SNAP) != 0;
    if (limit > nodes) limit = nodes;
    NRSCHK(blockTot.alloc(sizeof(uint32_t) * (size_t)mesh_blocks(nodes < MESH_BATCH ? nodes : MESH_BATCH)));
    NRSCHK(hdr.alloc(sizeof(MeshHeader)));
    NRSCHK(selIdx.alloc(sizeof(uint32_t) * (size_t)limit));
    if (snapped) NRSCHK(selQ.alloc(3 * sizeof(double) * (size_t)limit));
    HIPCHK(hipMemsetAsync(hdr.p, 0, sizeof(MeshHeader), stream));
    for (uint64_t b = 0; b < mesh_batches(nodes); ++b) {
        uint64_t first;
        uint32_t m;
        mesh_batch(nodes, b, first, m);
        NRSCHK(batch_field(L, first, m, S.useW != 0u, S.useD != 0u, stream));
        const uint32_t nb = mesh_blocks(m);
        hipLaunchKernelGGL(k_mesh_count, dim3(nb), dim3(MESH_BLOCK), 0, stream, S, (const double *)w.as<double>(), (const double *)d2.as<double>(), m,
                           blockTot.as<uint32_t>());
        hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(SCAN_BLOCK), 0, stream, blockTot.as<uint32_t>(), nb, hdr.as<MeshHeader>());
        if (limit)
            hipLaunchKernelGGL(k_mesh_compact, dim3(nb), dim3(MESH_BLOCK), 0, stream, S, (const double *)w.as<double>(), (const double *)d2.as<double>(),
                               (const double *)q.as<double>(), first, m, (const uint32_t *)blockTot.as<uint32_t>(),
                               (const MeshHeader *)hdr.as<MeshHeader>(), limit, selIdx.as<uint32_t>(), snapped ? selQ.as<double>() : nullptr);
        HIPCHK(hipGetLastError());
    }
    MeshHeader h = {};
    HIPCHK(hipMemcpyAsync(&h, hdr.p, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    *count = h.total;
    return NRS_OK;
}

int MeshSampler::positions(int precision, const Lattice &L, uint64_t count, void *pos4, hipStream_t stream)
{
    if (!count) return NRS_OK;
    const size_t bytes = (precision == 64 ? sizeof(double4) : sizeof(float4)) * (size_t)count;
    NRSCHK(pos.alloc(bytes));
    const dim3 grid(mesh_blocks(count)), block(MESH_BLOCK);
    const uint32_t *idx = selIdx.as<uint32_t>();
    const double *sq = snapped ? selQ.as<double>() : nullptr;
    if (precision == 64) hipLaunchKernelGGL((k_mesh_positions<double4, double>), grid, block, 0, stream, L, idx, sq, (uint32_t)count, pos.as<double4>());
    else hipLaunchKernelGGL((k_mesh_positions<float4, float>), grid, block, 0, stream, L, idx, sq, (uint32_t)count, pos.as<float4>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pos4, pos.p, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return NRS_OK;
}

static int mesh_check_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(NRS_E_NODEVICE, "no HIP device available: libnereus_hip has no CPU fallback");
    if (device >= ndev) return fail(NRS_E_INVALID, "device ordinal out of range");
    return NRS_OK;
}
// a device (checked by mesh_check_device) and a stream for the length of a context-free call
struct MeshCall {
    DeviceScope scope;
    hipStream_t st = nullptr;
    MeshSampler ms;
    explicit MeshCall(int device) : scope(device) {}
    ~MeshCall()
    {
        if (st) (void)hipStreamSynchronize(st);
        ms.release();
        if (st) (void)hipStreamDestroy(st);
    }
    int open()
    {
        if (!scope.ok()) return fail(NRS_E_HIP, "hipSetDevice failed");
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return NRS_OK;
    }
};

} // namespace nrs

using namespace nrs;

extern "C" int nrs_mesh_field(int device, const nrs_mesh *mesh, const nrs_lattice *lattice, double *winding, double *dist2, uint32_t *nearest,
                              double *closest3)
{
    NRSCHK(mesh_check_mesh(mesh));
    uint64_t nodes = 0;
    NRSCHK(sample_check_lattice(lattice, &nodes));
    if (!winding && !dist2 && !nearest && !closest3) return NRS_OK;
    NRSCHK(mesh_check_device(device));
    MeshCall c(device);
    NRSCHK(c.open());
    NRSCHK(c.ms.upload(*mesh, c.st));
    return c.ms.field(lattice_from(*lattice), nodes, winding, dist2, nearest, closest3, c.st);
}

extern "C" int nrs_mesh_particles(int device, int precision, const nrs_mesh *mesh, const nrs_lattice *lattice, const nrs_mesh_rule *rule, void *pos4,
                                  uint64_t capacity, uint64_t *count)
{
    if (count) *count = 0;
    NRSCHK(mesh_check_precision(precision));
    NRSCHK(mesh_check_mesh(mesh));
    uint64_t nodes = 0;
    NRSCHK(sample_check_lattice(lattice, &nodes));
    NRSCHK(mesh_check_rule(rule));
    NRSCHK(mesh_check_device(device));
    MeshCall c(device);
    NRSCHK(c.open());
    NRSCHK(c.ms.upload(*mesh, c.st));
    const Lattice L = lattice_from(*lattice);
    uint64_t sel = 0;
    NRSCHK(c.ms.select(L, nodes, *rule, pos4 ? capacity : 0, c.st, &sel));
    if (count) *count = sel;
    if (!pos4) return NRS_OK;
    if (sel > capacity) return fail(NRS_E_CAPACITY, "mesh particles: more nodes selected than capacity");
    return c.ms.positions(precision, L, sel, pos4, c.st);
}
