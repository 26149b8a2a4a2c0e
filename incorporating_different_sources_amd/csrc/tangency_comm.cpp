// tangency_comm.cpp - host layer of libtangency.so: the RCCL communicator and the gathers of the results to one rank.
#include <cstring>

#include "tangency_host.h"

using namespace tp_host;

namespace {

// root's receive buffers of a gather over `ranks` ranks
int ensure_gather_buffers(tp_batch_t b, int ranks) {
    const size_t nw = (size_t)b->W * b->p.k, ns = (size_t)b->W;
    int rc = ensure(b->h, b->gather_w, sizeof(double) * nw * ranks, "gathered weights");
    if (rc == TP_OK) rc = ensure(b->h, b->gather_s, sizeof(int32_t) * ns * ranks, "gathered statuses");
    return rc;
}

// one gather of the weights and one of the statuses to root, as one group on `st` (closed on failure too)
ncclResult_t issue_gather(tp_batch_t b, const double* src_weights, const int32_t* src_status, int root, hipStream_t st) {
    tp_handle_t h = b->h;
    const size_t nw = (size_t)b->W * b->p.k, ns = (size_t)b->W;
    const bool is_root = h->rank == root;
    ncclResult_t r = ncclGroupStart();
    if (r != ncclSuccess) return r;
    r = ncclGather(src_weights, is_root ? b->gather_w.p : nullptr, nw, ncclDouble, root, h->comm, st);
    if (r == ncclSuccess) r = ncclGather(src_status, is_root ? b->gather_s.p : nullptr, ns, ncclInt32, root, h->comm, st);
    const ncclResult_t closed = ncclGroupEnd();
    return r != ncclSuccess ? r : closed;
}

}  // namespace

// Put the requested gather (tp_batch_gather_async) on the gather stream.  Called with the NEXT kernel already
// queued (tp_batch_run) or when the caller waits anyway: the host waits for the end of the run whose results
// are gathered, so the gather stream needs no device-side wait for the kernel stream.
int tp_host::flush_gather(tp_handle_t h) {
    tp_batch_t b = h->deferred;
    if (!b || !b->gather_req) { h->deferred = nullptr; return TP_OK; }
    HIP_TRY(h, hipSetDevice(h->device));
    const int root = b->gather_root, par = b->gather_req_parity;
    HIP_TRY(h, hipEventSynchronize(b->snap));
    // the gather span: re-recorded only when the previous one has been read or is already complete
    const bool time_this = !h->gather_span.busy();
    if (time_this) HIP_TRY(h, h->gather_span.read(h->gather_ms));
    const double* sw = (const double*)(par ? b->weights2.p : b->weights.p);
    const int32_t* ss = (const int32_t*)(par ? b->status2.p : b->status.p);
    if (time_this) HIP_TRY(h, h->gather_span.begin(h->comm_stream));
    NCCL_TRY(h, issue_gather(b, sw, ss, root, h->comm_stream));
    if (time_this) HIP_TRY(h, h->gather_span.end(h->comm_stream));
    HIP_TRY(h, hipEventRecord(b->gather_done[par], h->comm_stream));
    b->gather_pending[par] = true;
    b->gather_req = false;
    h->deferred = nullptr;
    return TP_OK;
}

extern "C" {

int tp_comm_unique_id(void* id) {
    if (!id) return TP_ERR_INVALID;
    ncclUniqueId uid;
    if (ncclGetUniqueId(&uid) != ncclSuccess) return TP_ERR_RCCL;
    memcpy(id, &uid, sizeof uid);
    return TP_OK;
}

int tp_comm_init(tp_handle_t h, const void* id, int rank, int world) {
    if (!h || !id) return TP_ERR_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, TP_ERR_INVALID, "bad rank %d / world %d", rank, world);
    if (h->comm) return fail(h, TP_ERR_INVALID, "communicator already initialised");
    HIP_TRY(h, hipSetDevice(h->device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    NCCL_TRY(h, ncclCommInitRank(&h->comm, world, uid, rank));
    h->rank = rank;
    h->world = world;
    return TP_OK;
}

int tp_comm_count(tp_handle_t h, int* ranks) {
    if (!h || !ranks) return TP_ERR_INVALID;
    *ranks = 0;
    if (!h->comm) return fail(h, TP_ERR_INVALID, "tp_comm_count without a communicator");
    NCCL_TRY(h, ncclCommCount(h->comm, ranks));
    return TP_OK;
}

// Single-process form: one communicator over the n handles of this process (rank i = handles[i]), no id exchange
// and no launcher - what main.py (one process, src/main.py:26) can use on an 8-GPU node.
int tp_comm_init_all(tp_handle_t* handles, int n) {
    if (!handles || n < 1) return TP_ERR_INVALID;
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!handles[i]) return TP_ERR_INVALID;
        if (handles[i]->comm) return fail(handles[i], TP_ERR_INVALID, "communicator already initialised");
        devs[(size_t)i] = handles[i]->device;
        for (int j = 0; j < i; ++j)
            if (devs[(size_t)j] == devs[(size_t)i])
                return fail(handles[0], TP_ERR_INVALID, "tp_comm_init_all: handles %d and %d share device %d (one rank per GPU)", j, i, devs[(size_t)i]);
    }
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    NCCL_TRY(handles[0], ncclCommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; ++i) { handles[i]->comm = comms[(size_t)i]; handles[i]->rank = i; handles[i]->world = n; }
    return TP_OK;
}

// The gather of tp_batch_gather for the single-process communicator: batches[i] lives on rank i, all with the same
// W; every rank's ncclGather pair is issued inside ONE group (a single thread drives all the devices), each on its
// handle's kernel stream.  Waits for root's stream; the result stays in root's HBM and, with host buffers given,
// is copied out [n x W x k] / [n x W].
int tp_group_gather(tp_batch_t* batches, int n, int root, double* weights_all, int32_t* status_all) {
    if (!batches || n < 1 || root < 0 || root >= n) return TP_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        if (!batches[i]) return TP_ERR_INVALID;
        tp_handle_t h = batches[i]->h;
        if (!h->comm || h->world != n || h->rank != i)
            return fail(h, TP_ERR_INVALID, "tp_group_gather: batches[%d] is not on rank %d of an %d-rank communicator", i, i, n);
        if (batches[i]->W != batches[0]->W || batches[i]->p.k != batches[0]->p.k)
            return fail(h, TP_ERR_INVALID, "tp_group_gather: every rank must hold the same W and k");
    }
    tp_batch_t rb = batches[root];
    tp_handle_t rh = rb->h;
    HIP_TRY(rh, hipSetDevice(rh->device));
    int rc = ensure_gather_buffers(rb, n);
    if (rc != TP_OK) return rc;
    NCCL_TRY(rh, ncclGroupStart());
    for (int i = 0; i < n; ++i) {
        tp_batch_t b = batches[i];
        const ncclResult_t r = issue_gather(b, b->out_weights(), b->out_status(), root, b->h->stream);
        if (r != ncclSuccess) { (void)ncclGroupEnd(); return fail(rh, TP_ERR_RCCL, "ncclGather (rank %d) failed: %s", i, ncclGetErrorString(r)); }
    }
    NCCL_TRY(rh, ncclGroupEnd());
    for (int i = 0; i < n; ++i) {
        tp_handle_t h = batches[i]->h;
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        int rck = harvest_kernel_time(h);
        if (rck != TP_OK) return rck;
    }
    rb->gathered = true;
    if (weights_all || status_all) return tp_batch_download_gathered(rb, weights_all, status_all);
    return TP_OK;
}

int tp_comm_destroy(tp_handle_t h) {
    if (!h) return TP_ERR_INVALID;
    if (h->deferred) { int rcf = flush_gather(h); if (rcf != TP_OK) return rcf; }
    if (h->comm_stream) { HIP_TRY(h, hipSetDevice(h->device)); HIP_TRY(h, hipStreamSynchronize(h->comm_stream)); }
    if (h->comm) { NCCL_TRY(h, ncclCommDestroy(h->comm)); h->comm = nullptr; }
    h->world = 1; h->rank = 0;
    return TP_OK;
}

int tp_batch_gather(tp_batch_t b, int root, double* weights_all, int32_t* status_all) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!h->comm) return fail(h, TP_ERR_INVALID, "tp_batch_gather without tp_comm_init");
    if (root < 0 || root >= h->world) return fail(h, TP_ERR_INVALID, "bad root %d", root);
    HIP_TRY(h, hipSetDevice(h->device));
    // collectives of one communicator must be issued in the same order on every rank: a gather still waiting to
    // go onto the gather stream comes first, and this one only after it has finished there
    if (h->deferred) { int rcf = flush_gather(h); if (rcf != TP_OK) return rcf; }
    if (h->comm_stream) HIP_TRY(h, hipStreamSynchronize(h->comm_stream));
    const bool is_root = h->rank == root;
    if (is_root) {
        int rc = ensure_gather_buffers(b, h->world);
        if (rc != TP_OK) return rc;
    }
    Span span;                                         // of this call: the handle's gather span may still be unread
    HIP_TRY(h, span.create());
    HIP_TRY(h, span.begin(h->stream));
    NCCL_TRY(h, issue_gather(b, b->out_weights(), b->out_status(), root, h->stream));   // on the stream of the kernel
    HIP_TRY(h, span.end(h->stream));
    HIP_TRY(h, span.read(h->gather_ms));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    b->gathered = true;
    if (is_root && (weights_all || status_all)) return tp_batch_download_gathered(b, weights_all, status_all);
    return TP_OK;
}

int tp_batch_gather_async(tp_batch_t b, int root) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!h->comm) return fail(h, TP_ERR_INVALID, "tp_batch_gather_async without tp_comm_init");
    if (root < 0 || root >= h->world) return fail(h, TP_ERR_INVALID, "bad root %d", root);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->comm_stream.create_high_priority());
    HIP_TRY(h, h->gather_span.create());
    int rc = TP_OK;
    if (h->deferred) { rc = flush_gather(h); if (rc != TP_OK) return rc; }     // an earlier request nobody ran after
    if (!b->pingpong) {                                // first use: the second result pair and its events
        rc = ensure(h, b->weights2, sizeof(double) * (size_t)b->W * b->p.k, "second weights buffer");
        if (rc == TP_OK) rc = ensure(h, b->status2, sizeof(int32_t) * (size_t)b->W, "second status buffer");
        if (rc != TP_OK) return rc;
        for (Event& e : b->gather_done) HIP_TRY(h, e.create(hipEventDisableTiming));
        HIP_TRY(h, b->snap.create(hipEventDisableTiming));
        b->pingpong = true;
    }
    if (h->rank == root) rc = ensure_gather_buffers(b, h->world);
    if (rc != TP_OK) return rc;
    // Only a request: the gather goes onto its stream inside the NEXT tp_batch_run, after that run's kernel
    // is queued (or in tp_synchronize / tp_batch_download_gathered) - see flush_gather.
    HIP_TRY(h, hipEventRecord(b->snap, h->stream));
    b->gather_req = true;
    b->gather_req_parity = b->parity;
    b->gather_root = root;
    h->deferred = b;
    b->gathered = true;
    return TP_OK;
}

int tp_batch_download_gathered(tp_batch_t b, double* weights_all, int32_t* status_all) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!b->gathered || !b->gather_w.p) return fail(h, TP_ERR_INVALID, "nothing gathered on this rank (root only, after tp_batch_gather)");
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->deferred) { int rcf = flush_gather(h); if (rcf != TP_OK) return rcf; }
    if (h->comm_stream) {                              // an asynchronous gather may still be filling gather_w
        HIP_TRY(h, hipStreamSynchronize(h->comm_stream));
    }
    const size_t nw = (size_t)b->W * b->p.k, ns = (size_t)b->W;
    return download(h, {{weights_all, b->gather_w.p, sizeof(double) * nw * h->world},
                        {status_all, b->gather_s.p, sizeof(int32_t) * ns * h->world}});
}

}  // extern "C"