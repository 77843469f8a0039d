// hns_dist_substep.hip -- multi-GPU: the exchange (post / complete) and its kernels, and the core / full substep of a rank as a sequence of phases (see hns_dist.hpp).
// Three things are stated once here: how an exchange's fields lie in a message (lay_out; one pack / unpack kernel, k_halo_copy, launched by launch_halo_copy), how the
// messages travel (one transfer_* per hnsd::Transport, picked by transfer()), and which form a stencil phase takes (Step::stencil).
#include "hns_dist.hpp"

namespace hns {
using hnsd::kMaxBatchPeers;

// ---------------------------------------------------------------------------------------------------------------
// masked pack / unpack: one wave per listed leaf, lane = z-row (x*8+y), 8-bit z-mask per row
// ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int wave_exclusive_scan(int v) {
	int s = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const int t = __shfl_up(s, d, 64);
		if ((int)threadIdx.x >= d) s += t;
	}
	return s - v;
}

// loopback transport only: stands in for the time a message spends on the wire (option "dist_wire_us")
__global__ void k_wire_delay(long long ticks) {
	const long long t0 = wall_clock64();  // constant 100 MHz clock
	while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// One launch serves ALL peers of a rank (a rank of a 3-d decomposition talks to several: 7 in the 8-range plume): entry i carries its peer, whose message
// base and region size come by value. A null `peer` table: every entry is peer 0 (the tables of one peer's region).
struct PeerMsgs {
	float* base[kMaxBatchPeers];
	int voxels[kMaxBatchPeers];
};

template <int NCOMP, bool PACK>
__global__ __launch_bounds__(64) void k_halo_copy(float* __restrict__ field, const int* __restrict__ leaf, const unsigned char* __restrict__ mask,
                                                  const int* __restrict__ off, const int* __restrict__ peer, const PeerMsgs msgs, const int comps_before) {
	const int i = blockIdx.x, l = threadIdx.x;
	const unsigned m = mask[(size_t)i * 64 + l];
	const int p = peer ? peer[i] : 0;
	const int base = off[i] + wave_exclusive_scan(__popc(m));
	float* f = field + ((size_t)leaf[i] * 512 + l * 8) * NCOMP;
	float* q = msgs.base[p] + (size_t)comps_before * (size_t)msgs.voxels[p] + (size_t)base * NCOMP;
	int c = 0;
#pragma unroll
	for (int z = 0; z < 8; ++z) {
		if (m >> z & 1) {
#pragma unroll
			for (int k = 0; k < NCOMP; ++k) {
				if (PACK)
					q[c * NCOMP + k] = f[z * NCOMP + k];
				else
					f[z * NCOMP + k] = q[c * NCOMP + k];
			}
			++c;
		}
	}
}

// ---- one-sided transport (hipIpc-mapped peers): sequence-numbered flags (hns_flags.hpp), bounded waits ----
using hnsd::kIpcMaxSegs;
using hnsd::kIpcMaxPeers;

struct IpcPeers {
	int n;
	uint32_t* theirs_ready[kIpcMaxPeers];   // the peer's flag "rank <me> is ready to receive"   (in the PEER's memory)
	uint32_t* theirs_landed[kIpcMaxPeers];  // the peer's flag "what rank <me> sent has landed"   (in the PEER's memory)
	int rank[kIpcMaxPeers];
};

// "my receive side of exchange `seq` may be written": told to every peer; then wait for the same from every peer. One wave
// does all the waiting of a rank: waiting inside the copy kernel's workgroups filled the device with spinning waves (four
// processes of a 66k-leaf plume on one GPU: nothing else could be scheduled, every bounded wait ran out).
__global__ void k_ipc_ready(const IpcPeers peers, const uint32_t* __restrict__ my_flags, const uint32_t seq, int* status) {
	if ((int)threadIdx.x < peers.n) {
		flag_store(peers.theirs_ready[threadIdx.x], seq);
		flag_wait(my_flags + peers.rank[threadIdx.x], seq, status);
	}
}

struct IpcSegs {
	int n;
	float* dst[kIpcMaxSegs];  // in the peer's memory
	const float* src[kIpcMaxSegs];
	unsigned floats[kIpcMaxSegs];
	unsigned wg0[kIpcMaxSegs + 1];  // first workgroup of every segment
};

// Copies the segments into the peers' memory, 4,096 floats per workgroup (the receivers are ready: k_ipc_ready ran).
template <bool FENCE>  // (FENCE: the destination is another process's / device's memory; false: the loopback stand-in, this rank's own buffers)
__global__ __launch_bounds__(256) void k_ipc_put(const IpcSegs segs) {
	int s = 0;
	while (s + 1 < segs.n && blockIdx.x >= segs.wg0[s + 1]) ++s;
	const size_t first = (size_t)(blockIdx.x - segs.wg0[s]) * 4096u;
	const unsigned n = segs.floats[s];
	const float* __restrict__ src = segs.src[s];
	float* __restrict__ dst = segs.dst[s];
	if ((((uintptr_t)src | (uintptr_t)dst) & 15u) == 0 && (n & 3u) == 0) {
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const size_t i = first + ((size_t)j * 256u + threadIdx.x) * 4u;
			if (i < n) *(float4*)(dst + i) = *(const float4*)(src + i);
		}
	} else {
#pragma unroll 4
		for (int j = 0; j < 16; ++j) {
			const size_t i = first + (size_t)j * 256u + threadIdx.x;
			if (i < n) dst[i] = src[i];
		}
	}
	if (FENCE) __threadfence_system();
}

// after the puts (kernel boundary + fence): tell every peer its message has landed, then wait for theirs
__global__ void k_ipc_landed(const IpcPeers peers, const uint32_t* __restrict__ my_flags, const uint32_t seq, int* status) {
	__threadfence_system();
	if ((int)threadIdx.x < peers.n) {
		flag_store(peers.theirs_landed[threadIdx.x], seq);
		flag_wait(my_flags + kFlagLanded + peers.rank[threadIdx.x], seq, status);
	}
}

// Chained substep, the two advection kernels: they run as they are (512 threads per leaf at a 64-register cap: the chain code
// inside them cost three spilled registers and 25 % of their speed, measured) between a one-wave gate (k_sweep_wait: "peers,
// my previous launch is complete" + wait for theirs) and this kernel, which copies what the peers read of the boundary
// leaves' new values into the peers' ghost voxels: one wave per boundary leaf, lane = z-row.
template <int NC>
__global__ __launch_bounds__(64) void k_chain_mirror(const PhaseMirror m, const int n_out, const float* f0, const float* f1, const float* f2, const float* f3,
                                                     const float* f4, const float* f5, const float* f6, const float* f7) {
	const int leaf = blockIdx.x, l = threadIdx.x;
	const float* fields[8] = {f0, f1, f2, f3, f4, f5, f6, f7};
	const int e1 = m.first[leaf + 1];
	for (int e = m.first[leaf]; e < e1; ++e) {
		const int2 t = m.entry[e];
		const unsigned bits = m.mask ? m.mask[(size_t)e * 64 + l] : 0xFFu;
		if (!bits) continue;
#pragma unroll 1
		for (int o = 0; o < n_out; ++o) {
			const float* src = fields[o] + ((size_t)leaf * 512 + l * 8) * NC;
			float* dst = chain_out(m, t.x, o) + ((size_t)t.y * 512 + l * 8) * NC;
			if (bits == 0xFFu) {
#pragma unroll
				for (int q = 0; q < 2 * NC; ++q) store_through(dst + 4 * q, *reinterpret_cast<const float4*>(src + 4 * q));
			} else {
#pragma unroll
				for (int z = 0; z < 8; ++z)
					if (bits >> z & 1) {
#pragma unroll
						for (int c = 0; c < NC; ++c) store_through(dst + z * NC + c, src[z * NC + c]);
					}
			}
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// mirror pressure loop: a rank without boundary waves still tells its peers that its sweep is complete; and, after the last
// sweep of a solve, a rank waits for its peers' before the gradient kernel reads the ghost voxels they wrote
__global__ void k_sweep_signal(const PhaseMirror m) {
	if ((int)threadIdx.x < m.n_peers) flag_store(m.peer_flag[threadIdx.x], m.seq);
}
__global__ void k_sweep_wait(const PhaseMirror m) {  // (raises this rank's flag for m.seq first: its sweeps up to m.seq have ended)
	if ((int)threadIdx.x < m.n_peers) {
		flag_store(m.peer_flag[threadIdx.x], m.seq);
		flag_wait(m.my_flags + kFlagSweep + m.peer_rank[threadIdx.x], m.seq, m.status);
	}
}

}  // namespace hns

using namespace hns;
using namespace hnsd;

// ---------------------------------------------------------------------------------------------------------------
// exchange: post (pack, hand to the communication stream) / complete (wait, unpack)
// ---------------------------------------------------------------------------------------------------------------

namespace {

typedef std::vector<MsgField> Fields;

// statistics: `comps` floats per voxel of every peer's send region of type `t` leave this rank; returns how many peers get any
int count_sent(hns_dist* d, int t, int comps) {
	int messages = 0;
	for (const Peer& p : d->peers) {
		const size_t fl = (size_t)comps * (size_t)p.send[t].voxels;
		d->bytes_sent[t] += sizeof(float) * fl, messages += fl != 0;
	}
	return messages;
}

// the arguments of one chained launch: region type `t`, output arrays `outs` (device fields of this rank, components per voxel)
PhaseMirror phase_args(hns_dist* d, int t, const Fields& outs) {
	PhaseMirror m = d->mir;
	m.first = d->mir_type[t].first, m.entry = d->mir_type[t].entry, m.mask = d->mir_type[t].mask;
	int k = 0, comps = 0;
	for (const MsgField& f : outs) m.out_unit[k++] = (int)((size_t)((const char*)f.field - d->arena.as<const char>()) / d->unit_bytes), comps += f.ncomp;
	m.seq = ++d->sweep_seq;
	count_sent(d, t, comps);
	return m;
}

// THE layout of a message, stated here once: the exchange's fields in order, field f starting f.before * region.voxels floats into every peer's message.
// Whoever reads or writes a message -- pack / unpack, the transfers, message_floats -- goes by f.before (and segment()).
void lay_out(Pending& x) {
	int before = 0;
	for (MsgField& f : x.fields) f.before = before, before += f.ncomp;
	x.comps = before;
}

// The one place the pack / unpack kernel is launched: `n` table entries of `field`, whose messages are `msgs` (`peer`: see k_halo_copy).
void launch_halo_copy(bool pack, float* field, int ncomp, size_t n, const int* leaf, const unsigned char* mask, const int* off, const int* peer, const PeerMsgs& msgs,
                      int comps_before, hipStream_t st) {
	const dim3 grid((unsigned)n), block(64);
	if (ncomp == 3) {
		if (pack)
			hipLaunchKernelGGL((k_halo_copy<3, true>), grid, block, 0, st, field, leaf, mask, off, peer, msgs, comps_before);
		else
			hipLaunchKernelGGL((k_halo_copy<3, false>), grid, block, 0, st, field, leaf, mask, off, peer, msgs, comps_before);
	} else {
		if (pack)
			hipLaunchKernelGGL((k_halo_copy<1, true>), grid, block, 0, st, field, leaf, mask, off, peer, msgs, comps_before);
		else
			hipLaunchKernelGGL((k_halo_copy<1, false>), grid, block, 0, st, field, leaf, mask, off, peer, msgs, comps_before);
	}
}

// one field of one peer's region; `msg`: where that field starts in the peer's message
int halo_copy(bool pack, float* field, int ncomp, const Region& r, float* msg, hipStream_t st) {
	if (r.leaf.empty()) return HNS_OK;
	if (r.whole) return pack ? hns_dev_pack_leaves(field, r.d_leaf, r.leaf.size(), msg, ncomp, st) : hns_dev_unpack_leaves(msg, r.d_leaf, r.leaf.size(), field, ncomp, st);
	PeerMsgs one{};
	one.base[0] = msg, one.voxels[0] = r.voxels;
	launch_halo_copy(pack, field, ncomp, r.leaf.size(), r.d_leaf, r.d_mask, r.d_off, nullptr, one, 0, st);
	return launch_status("hns_dist: halo pack/unpack");
}

// every field of exchange `x`, all peers: one launch per field where the combined tables exist, per peer otherwise
int halo_copy_exchange(hns_dist* d, bool pack, const Pending& x, hipStream_t st) {
	const hns_dist::AllPeers& a = pack ? d->all_send[x.type] : d->all_recv[x.type];
	if (a.d_leaf) {
		if (a.n == 0) return HNS_OK;
		PeerMsgs msgs;
		for (size_t pi = 0; pi < d->peers.size(); ++pi) {
			msgs.base[pi] = pack ? d->peers[pi].sbuf[x.parity] : d->peers[pi].rbuf[x.parity];
			msgs.voxels[pi] = (pack ? d->peers[pi].send[x.type] : d->peers[pi].recv[x.type]).voxels;
		}
		for (const MsgField& f : x.fields) launch_halo_copy(pack, f.field, f.ncomp, (size_t)a.n, a.d_leaf, a.d_mask, a.d_off, a.d_peer, msgs, f.before, st);
		return launch_status("hns_dist: halo pack/unpack");
	}
	for (Peer& p : d->peers) {
		float* msg = pack ? p.sbuf[x.parity] : p.rbuf[x.parity];
		const Region& r = pack ? p.send[x.type] : p.recv[x.type];
		if (r.direct >= 0) continue;
		for (const MsgField& f : x.fields) HNS_TRY(halo_copy(pack, f.field, f.ncomp, r, msg + (size_t)f.before * (size_t)r.voxels, st));
	}
	return HNS_OK;
}

// where field `f` of a message lives: in the field itself when the region is a run of whole consecutive leaves, in the message buffer `buf` otherwise
// (`field`: the array of that field on the rank whose region `r` is -- f.field on this rank)
float* segment(const Region& r, const MsgField& f, float* field, float* buf) {
	return r.direct >= 0 ? field + (size_t)r.direct * 512 * (size_t)f.ncomp : buf + (size_t)f.before * (size_t)r.voxels;
}

size_t message_floats(const Pending& x, const Region& r) { return (size_t)x.comps * (size_t)r.voxels; }

// All messages of exchange `x` as k_ipc_put launches of up to kIpcMaxSegs segments on its stream, one segment per peer and field: `voxels(i)` voxels of peer i's send
// region travel, and field `f` of that message lands at `dst(i, f)`.
template <bool FENCE, class VoxelsFn, class DstFn>
void put_messages(hns_dist* d, const Pending& x, VoxelsFn voxels, DstFn dst) {
	IpcSegs sg;
	sg.n = 0, sg.wg0[0] = 0;
	auto flush = [&]() {
		if (sg.n) hipLaunchKernelGGL(k_ipc_put<FENCE>, dim3(sg.wg0[sg.n]), dim3(256), 0, x.stream, sg);
		sg.n = 0;
	};
	for (size_t i = 0; i < d->peers.size(); ++i) {
		const Peer& p = d->peers[i];
		for (const MsgField& f : x.fields) {
			const size_t fl = voxels(i) * (size_t)f.ncomp;
			if (!fl) continue;
			if (sg.n == kIpcMaxSegs) flush();
			sg.dst[sg.n] = dst(i, f), sg.src[sg.n] = segment(p.send[x.type], f, f.field, p.sbuf[x.parity]), sg.floats[sg.n] = (unsigned)fl;
			sg.wg0[sg.n + 1] = sg.wg0[sg.n] + (unsigned)((fl + 4095) / 4096);
			++sg.n;
		}
	}
	flush();
}

// ---- the transfer of a posted (packed) exchange, one function per transport, all on the exchange's stream ----

// ipc: "ready to receive" both ways, the puts into the peers' memory, "landed" both ways
int transfer_ipc(hns_dist* d, const Pending& x) {
	const uint32_t seq = ++d->ipc_seq;
	IpcPeers ip;
	ip.n = (int)d->peers.size();
	for (int i = 0; i < ip.n; ++i) {
		ip.theirs_ready[i] = d->ipc_peers[(size_t)i].flags + d->rank;
		ip.theirs_landed[i] = d->ipc_peers[(size_t)i].flags + kFlagLanded + d->rank;
		ip.rank[i] = d->peers[(size_t)i].rank;
	}
	hipLaunchKernelGGL(k_ipc_ready, dim3(1), dim3(64), 0, x.stream, ip, (const uint32_t*)d->ipc_flags, seq, d->ipc_status);
	put_messages<true>(d, x, [&](size_t i) { return (size_t)d->peers[i].send[x.type].voxels; }, [&](size_t i, const MsgField& f) {
		// the same field in the peer's memory: fields sit at the same multiples of the (peer's) unit
		const hns_dist::IpcPeer& q = d->ipc_peers[i];
		const size_t unit_index = (size_t)((char*)f.field - d->arena.as<char>()) / d->unit_bytes;
		return (float*)(q.recv_direct[x.type] >= 0 ? q.arena + unit_index * q.unit_bytes + sizeof(float) * 512 * (size_t)q.recv_direct[x.type] * (size_t)f.ncomp
		                                           : q.tables + q.rbuf_off[x.parity] + sizeof(float) * (size_t)f.before * (size_t)q.recv_voxels[x.type]);
	});
	hipLaunchKernelGGL(k_ipc_landed, dim3(1), dim3(64), 0, x.stream, ip, (const uint32_t*)d->ipc_flags, seq, d->ipc_status);
	return launch_status("hns_dist: one-sided exchange");
}

// RCCL: sends and receives of all peers are one group
int transfer_rccl(hns_dist* d, const Pending& x) {
	HNS_NCCL(rccl().GroupStart());
	for (Peer& p : d->peers) {
		const Region &rs = p.send[x.type], &rr = p.recv[x.type];
		// (loopback over RCCL: the peer is this rank, the answer to a message is the message, cut to the smaller region)
		const int to = d->loopback ? 0 : p.rank;
		const size_t vs = d->loopback ? (size_t)std::min(rs.voxels, rr.voxels) : (size_t)rs.voxels, vr = d->loopback ? vs : (size_t)rr.voxels;
		for (const MsgField& f : x.fields) {  // one send and one receive per field: either end may use the field itself or its buffer
			if (vs) HNS_NCCL(rccl().Send(segment(rs, f, f.field, p.sbuf[x.parity]), vs * f.ncomp, ncclFloat, to, d->comm, x.stream));
			if (vr) HNS_NCCL(rccl().Recv(segment(rr, f, f.field, p.rbuf[x.parity]), vr * f.ncomp, ncclFloat, to, d->comm, x.stream));
		}
	}
	HNS_NCCL(rccl().GroupEnd());
	return HNS_OK;
}

// loopback: same streams, events and copy sizes as a real exchange, but the payload is this rank's own
int transfer_loopback(hns_dist* d, const Pending& x) {
	if (const int us = options().dist_wire_us.load()) hipLaunchKernelGGL(k_wire_delay, dim3(1), dim3(1), 0, x.stream, (long long)us * 100);
	// all messages of the exchange as ONE copy launch (round 6; a hipMemcpyAsync per peer and field cost the host 5-8 us each, two to fourteen of them per exchange):
	// what stands in for the one send / receive group of the RCCL path
	put_messages<false>(d, x, [&](size_t i) { return (size_t)std::min(d->peers[i].send[x.type].voxels, d->peers[i].recv[x.type].voxels); },
	                    [&](size_t i, const MsgField& f) { return segment(d->peers[i].recv[x.type], f, f.field, d->peers[i].rbuf[x.parity]); });
	return launch_status("hns_dist: loopback exchange");
}

// local: nothing travels at post(); at complete() this rank pulls every peer's message out of its send buffer, once the peer has packed it
int transfer_local(hns_dist* d, const Pending& x) {
	for (Peer& p : d->peers) {
		// the peer packed this message into its buffer of the same parity when it posted the same exchange; it may already
		// have posted the NEXT one (other parity) -- never the one after, which its own complete() of this one precedes
		hns_dist* q = d->local_ranks[(size_t)p.rank];
		const Peer* back = nullptr;
		for (const Peer& c : q->peers)
			if (c.rank == d->rank) back = &c;
		const size_t nr = message_floats(x, p.recv[x.type]);
		if (!nr) continue;
		if (!back || message_floats(x, back->send[x.type]) != nr) return fail(HNS_ERR_RUNTIME, "hns_dist: send/receive plans of two ranks disagree");
		const Pending& y = q->pending;  // the peer's record of the same exchange (its fields are ITS device arrays)
		if (y.type != x.type || y.parity != x.parity || y.fields.size() != x.fields.size()) return fail(HNS_ERR_RUNTIME, "hns_dist: locally connected ranks are out of step");
		if (!d->single_stream) HNS_HIP(hipStreamWaitEvent(x.stream, q->ev_post[x.parity], 0));
		for (size_t fi = 0; fi < x.fields.size(); ++fi) {
			const MsgField& f = x.fields[fi];
			HNS_HIP(hipMemcpyAsync(segment(p.recv[x.type], f, f.field, p.rbuf[x.parity]), segment(back->send[x.type], f, y.fields[fi].field, back->sbuf[x.parity]),
			                       sizeof(float) * (size_t)p.recv[x.type].voxels * f.ncomp, hipMemcpyDeviceToDevice, x.stream));
		}
	}
	return HNS_OK;
}

int transfer(hns_dist* d, const Pending& x, Transport via) {
	switch (via) {
		case Transport::Ipc: return transfer_ipc(d, x);
		case Transport::Rccl: return transfer_rccl(d, x);
		case Transport::Loopback: return transfer_loopback(d, x);
		default: return HNS_OK;  // (local: transfer_local, from complete())
	}
}

// received regions -> ghost voxels, on the communication stream; ev_done marks the end of the exchange
int unpack(hns_dist* d, Pending& x) {
	HNS_TRY(halo_copy_exchange(d, false, x, x.stream));
	if (!d->single_stream) HNS_HIP(hipEventRecord(d->ev_done[x.parity], x.stream));
	return HNS_OK;
}

const auto nothing = [](hipStream_t) { return (int)HNS_OK; };  // a boundary or interior launch that has nothing to launch
const auto no_chain = [](const PhaseMirror&) { return fail(HNS_ERR_RUNTIME, "hns_dist: this phase has no chained form"); };  // (a phase of the full substep only)

// One exchange. post(): the compute stream `st` marks "everything the boundary kernel reads is ready", and the rank's
// communication stream takes over the whole boundary side of the step: `boundary(cs)` runs the kernel on the boundary leaves,
// the regions the peers read are packed, the messages travel, the received regions are unpacked into the ghost voxels. The
// caller then launches the interior kernel on `st`, which runs concurrently with all of that (an interior leaf touches no
// ghost and no ghost-facing leaf writes what it reads). complete(): `st` waits for the end of that chain.
// The messages travel by transfer(): one function per transport (local: the peers pull at complete()).
// Round 6: `interior(st)` -- the same kernel over the interior leaves -- is handed in and enqueued HERE, right behind the boundary kernel and in front of the pack / transfer /
// unpack calls. Enqueued after them (rounds 2-5) it reached the device only once the host had issued the whole boundary chain, and by then that chain had run: the two
// streams never overlapped (profiles/r06_dist_exchanged_timeline_before.txt; the loop is bound by the HOST's ~10 runtime calls per exchange).
// in_line: the whole exchange -- `boundary(st)`, pack, transfer, unpack -- on the compute stream itself, in order, no events, complete on return (round 6: the pressure loop
// whose one launch over all owned leaves packs its own messages; also what locally connected ranks do).
template <class BoundaryFn, class InteriorFn>
int post(hns_dist* d, int type, Fields fields, hipStream_t st, BoundaryFn boundary, InteriorFn interior, bool in_line = false) {
	if (d->pending.active) return fail(HNS_ERR_RUNTIME, "hns_dist: an exchange is already in flight");
	if (d->world == 1) {  // nobody to talk to: the boundary range is empty, keep everything on one stream
		HNS_TRY(boundary(st));
		return interior(st);
	}
	const Transport via = transport(d);
	if (via == Transport::None) return fail(HNS_ERR_RUNTIME, "hns_dist: not connected (call hns_dist_connect_rccl, hns_dist_connect_ipc or hns_dist_connect_local first)");
	Pending& x = d->pending;
	x.active = true, x.type = type, x.parity = d->parity, x.fields = std::move(fields);
	lay_out(x);
	d->parity ^= 1;
	const bool one_stream = d->single_stream || in_line;
	const hipStream_t cs = one_stream ? st : d->cs;
	x.stream = cs;
	if (!one_stream) {
		HNS_HIP(hipEventRecord(d->ev_ready, st));
		HNS_HIP(hipStreamWaitEvent(cs, d->ev_ready, 0));
	}
	x.prepacked = false;
	HNS_TRY(boundary(cs));
	if (!one_stream) HNS_HIP(hipEventRecord(d->ev_bdone[x.parity], cs));
	HNS_TRY(interior(st));
	if (!x.prepacked) HNS_TRY(halo_copy_exchange(d, true, x, cs));
	else ++d->packed_exchanges;
	d->messages_sent += (uint64_t)count_sent(d, type, x.comps);
	++d->exchanges;
	if (via == Transport::Local) {
		if (!d->single_stream) HNS_HIP(hipEventRecord(d->ev_post[x.parity], cs));  // packed: the peers may pull
		return HNS_OK;
	}
	HNS_TRY(transfer(d, x, via));
	if (in_line && !d->single_stream) {  // received regions -> ghost voxels behind the transfer on the same stream: nothing left to wait for
		HNS_TRY(halo_copy_exchange(d, false, x, cs));
		x.active = false;
		return HNS_OK;
	}
	return unpack(d, x);
}

// Make the posted exchange's data visible in the ghost voxels before anything else runs on the compute stream.
int complete(hns_dist* d, hipStream_t st) {
	Pending& x = d->pending;
	if (!x.active) return HNS_OK;
	if (transport(d) == Transport::Local) {
		HNS_TRY(transfer_local(d, x));
		HNS_TRY(unpack(d, x));
	}
	if (!d->single_stream) HNS_HIP(hipStreamWaitEvent(st, d->ev_done[x.parity], 0));
	x.active = false;
	return HNS_OK;
}

// Between two blocks of the exchanged pressure loop that sweep owned leaves only: the compute stream needs the boundary KERNEL of the posted exchange (interior tiles read the
// boundary leaves' new p), not its messages -- the ghost voxels are read by the next boundary kernel alone, which follows the unpack in stream order on the communication
// stream. So the compute stream waits for ev_bdone, the exchange is forgotten, and no cross-stream edge is left on the chain boundary sweep -> transfer -> unpack -> next
// boundary sweep. (The last exchange of a solve is completed in full by the phase behind it.) Two-stream transports only; false = the caller must complete() in full.
// Invariant (checked by build_plan): every interior leaf has all 26 neighbours absent or owned, and sweeps_per_exchange k <= 4. The interior launch may then run while the
// previous exchange's unpack is still writing ghost leaves: no interior voxel reads a ghost voxel, and the blocked sweep's dependency cone (2k <= 8 voxels) stays inside one leaf,
// so what an interior launch reads within a block is owned.
bool complete_boundary_only(hns_dist* d, hipStream_t st) {
	Pending& x = d->pending;
	if (!x.active) return true;
	if (!two_stream_transport(d)) return false;
	if (hipStreamWaitEvent(st, d->ev_bdone[x.parity], 0) != hipSuccess) return false;
	x.active = false;
	return true;
}

// ---------------------------------------------------------------------------------------------------------------
// the core / full substep as a list of phases; a phase ends where an exchange has been posted
// ---------------------------------------------------------------------------------------------------------------

enum class PhaseKind { Open, Collision, AdvectVector, Vorticity, Divergence, Combustion, SorBlock, Gradient, AdvectScalars };
struct Phase {
	PhaseKind kind;
	int block;  // SorBlock: which block of up to k sweeps of the pressure loop (0 otherwise)
	bool operator==(const Phase& o) const { return kind == o.kind && block == o.block; }
};

struct Step {
	hns_dist* d;
	int iterations;
	float dt;
	hipStream_t st;
	// pressure loop cursor
	int it = 0;
	float *src = nullptr, *dst = nullptr;
	// the whole Compute_Sim substep (reference HNanoSolver.cu:150-356) instead of its core: combustion parameters, the positions of
	// fuel / waste / temperature / flame / collision_sdf among the rank's scalars, collision on, vorticity confinement on
	const hns_combustion_params* prm = nullptr;
	int fi[5] = {-1, -1, -1, -1, -1};
	bool coll = false, vort = false;

	bool full() const { return prm != nullptr; }
	const float* sdf() const { return coll ? d->phi[(size_t)fi[4]] : nullptr; }
	float inv_dx() const { return 1.0f / d->voxel_size; }
	// Only the core substep takes the chained form (and the mirror pressure loop): the full one exchanges at every kernel boundary a stencil crosses, whatever the transport.
	bool chained_form() const { return !full() && d->chain; }
	bool exchanged_blocks() const { return full() || !d->mirror; }  // the pressure loop's blocks are sor_block_exchanged's (else mirror_block's)

	// open | [collision] | advect_vector | [vorticity] | divergence | [combustion] | blocks of up to k sweeps | gradient | advect_scalars (the core: none of [...])
	std::vector<Phase> phases() const {
		std::vector<Phase> p{{PhaseKind::Open, 0}};
		if (coll) p.push_back({PhaseKind::Collision, 0});
		p.push_back({PhaseKind::AdvectVector, 0});
		if (vort) p.push_back({PhaseKind::Vorticity, 0});
		p.push_back({PhaseKind::Divergence, 0});
		if (full()) p.push_back({PhaseKind::Combustion, 0});
		for (int b = 0, blocks = (iterations + d->k - 1) / d->k; b < blocks; ++b) p.push_back({PhaseKind::SorBlock, b});
		p.push_back({PhaseKind::Gradient, 0});
		p.push_back({PhaseKind::AdvectScalars, 0});
		return p;
	}

	// The one completion rule: a phase first makes the exchange in flight visible (complete), except Open -- it posts the first exchange of the substep -- and a
	// block of the exchanged pressure loop, which completes for itself (sor_block_exchanged: in full, or the boundary kernel alone). The mirror loop's blocks do complete first.
	int run(const Phase& p) {
		if (p.kind != PhaseKind::Open && !(p.kind == PhaseKind::SorBlock && exchanged_blocks())) HNS_TRY(complete(d, st));
		switch (p.kind) {
			case PhaseKind::Open: return open();
			case PhaseKind::Collision: return collision();
			case PhaseKind::AdvectVector: return advect_vector();
			case PhaseKind::Vorticity: return vorticity();
			case PhaseKind::Divergence: return divergence();
			case PhaseKind::Combustion: return combustion();
			case PhaseKind::SorBlock: return exchanged_blocks() ? sor_block_exchanged(p.block) : mirror_block(p.block);
			case PhaseKind::Gradient: return gradient();
			case PhaseKind::AdvectScalars: return advect_scalars();
		}
		return fail(HNS_ERR_RUNTIME, "hns_dist: unknown phase");
	}

	// Round 6: a SMALL rank (up to 16,384 owned leaves: BASELINE config 5 in 8 ranks has 8,243 each) runs its short phases -- the sweeps of the pressure loop, the divergence,
	// the gradient subtraction -- as ONE launch over all owned leaves with the exchange behind it on the compute stream (post(..., in_line)): at that size the boundary chain
	// (boundary kernel -> pack -> transfer -> unpack, each a latency-bound launch, plus two cross-stream event edges) is longer than the interior kernel it was meant to hide
	// under. Large ranks (a 256^3 slab: 32,768 leaves) keep the boundary / interior split on two streams. A rank decides for itself: the messages are the same either way.
	bool in_line_rank() const {
		const int u = options().dist_unsplit.load();  // 0 never | 1 by size | 2 always
		return two_stream_transport(d) && u != 0 && (u == 2 || d->nB + d->nI <= 16384);
	}

	// Do both launch ranges of the split sweep take two iterations in ONE launch each (result in dst for both)? Asked of the schedule
	// hns_rbgs_iterate walks, so that whatever it does with `2` is what this loop assumes.
	bool split_blocked() const {
		if (d->k < 2) return false;
		for (hns_grid* g : {d->gB, d->gI}) {
			if (!g->n_active) continue;
			if (!hns_rbgs_schedule(g, 2).one_blocked_launch()) return false;
		}
		return true;
	}

	// One chained launch (hns_flags.hpp: PhaseMirror): `launch` runs the kernel over the owned leaves with the arguments `m`.
	template <class Launch>
	int chained(const PhaseMirror& m, Launch launch, bool gate = false) {
		if ((gate || options().dist_mirror.load() == 2) && m.n_peers) {
			// "guarded": ONE wave waits for the peers' previous launch in front of this one, so that no boundary workgroup ever
			// spins. For ranks that share a GPU (tests, bench.py --share-one-gpu): there the boundary waves of several processes
			// waiting inside their kernels can occupy every wave slot of the device, and the process they all wait for is never
			// scheduled (four 16k-leaf plume ranks: every bounded wait ran out). ~5 us per launch.
			PhaseMirror w = m;
			w.seq = m.seq - 1u;
			hipLaunchKernelGGL(k_sweep_wait, dim3(1), dim3(64), 0, st, w);
		}
		if (d->gO->n_active) {
			HNS_TRY(launch());
			// (locally connected ranks share ONE stream: a rank's flag must not wait for its next launch, which sits behind the
			// peers' launches that wait for the flag)
			if (d->single_stream && m.n_peers) hipLaunchKernelGGL(k_sweep_signal, dim3(1), dim3(64), 0, st, m);
		} else if (m.n_peers) {  // a rank without leaves still takes part in the chain of flags
			hipLaunchKernelGGL(k_sweep_signal, dim3(1), dim3(64), 0, st, m);
		}
		return launch_status("hns_dist: chained launch");
	}

	// chained form of the two advection phases: behind the kernel as it is, the boundary leaves' new values go into the peers' ghost voxels (k_chain_mirror)
	template <int NC>
	int chain_mirror(const PhaseMirror& m, float* const* outs, int n_out) {
		const float* f[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
		for (int s = 0; s < n_out && s < 8; ++s) f[s] = outs[s];
		if (d->nB && m.n_peers) hipLaunchKernelGGL(k_chain_mirror<NC>, dim3((unsigned)d->nB), dim3(64), 0, st, m, n_out, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
		return HNS_OK;
	}

	// THE form of a stencil phase, chosen here for all of them. A phase states its kernel -- `kernel(g, s)`: over launch range g on stream s, an empty range being a no-op --,
	// the fields it writes that the peers read, and their region type; and `chain(m)`, its one launch over the owned leaves in the chained form (arguments m).
	//   chained   one launch over gO that delivers its own halo (the two advection kernels: behind a gate, with chain_mirror behind them)
	//   in line   one launch over gO, the exchange behind it on the compute stream: the SHORT phases of a small rank (in_line_rank), core substep only
	//   split     gB on the communication stream, gI handed to post(), which enqueues it in front of the pack / transfer / unpack calls
	//   the same with gI launched here, BEHIND post(): the full substep's divergence, gradient and scalar advection
	template <class Kernel, class Chain>
	int stencil(PhaseKind kind, int type, Fields fields, Kernel kernel, Chain chain) {
		const bool advection = kind == PhaseKind::AdvectVector || kind == PhaseKind::AdvectScalars;
		const bool short_phase = kind == PhaseKind::Divergence || kind == PhaseKind::Gradient;
		if (chained_form()) {
			const PhaseMirror m = phase_args(d, type, fields);
			return chained(m, [&] { return chain(m); }, advection);
		}
		auto over = [&kernel](hns_grid* g) { return [&kernel, g](hipStream_t s) { return kernel(g, s); }; };
		if (!full() && short_phase && in_line_rank()) return post(d, type, std::move(fields), st, over(d->gO), nothing, true);
		// The full substep's interior launch of these phases stays BEHIND post(). Moving it in front, as round 6 did for the core substep (see post()), changes the order
		// in which work reaches the device and so its timing: a performance change that needs its own measurement, not a refactor.
		const bool interior_behind_post = full() && (short_phase || kind == PhaseKind::AdvectScalars);
		if (interior_behind_post) {
			HNS_TRY(post(d, type, std::move(fields), st, over(d->gB), nothing));
			return kernel(d->gI, st);
		}
		return post(d, type, std::move(fields), st, over(d->gB), over(d->gI));
	}

	// the advection inputs: phi unless the previous substep already posted it, and u
	int open() {
		Fields f;
		if (full()) {  // (u may still need posting behind a phi in flight -- unless collision is about to rewrite u and post it again)
			if (!coll && !d->u_ghosts_fresh) {
				if (d->phi_in_flight) HNS_TRY(complete(d, st));
				f.emplace_back(d->u, 3);
			}
			if (!d->phi_in_flight)
				for (float* p : d->phi) f.emplace_back(p, 1);
			d->phi_in_flight = false;
		} else {  // (the core substep's last phase leaves u's ghosts fresh whenever it posts phi: nothing to add then)
			if (d->phi_in_flight) return HNS_OK;
			if (!d->u_ghosts_fresh) f.emplace_back(d->u, 3);
			for (float* p : d->phi) f.emplace_back(p, 1);
		}
		return f.empty() ? (int)HNS_OK : post(d, X_ADV, f, st, nothing, nothing);
	}

	// enforceCollisionBoundaries (HNanoSolver.cu:153-157) reads the ghost voxels of the SDF (its normal): they have arrived now
	int collision() {
		HNS_TRY(hns_dev_enforce_collision_boundaries(d->gO, d->u, sdf(), d->voxel_size, st));
		return post(d, X_ADV, Fields{{d->u, 3}}, st, nothing, nothing);
	}

	// advect_vector (:162-170); vorticity confinement reads it up to factor_scale + 1 voxels away: whole leaves travel then
	int advect_vector() {
		const float ix = inv_dx();
		auto kernel = [&](hns_grid* g, hipStream_t s) { return hns_dev_advect_vector(g, d->u, d->adv, sdf(), coll ? 1 : 0, dt, ix, s); };
		return stencil(PhaseKind::AdvectVector, vort ? X_ADV : X_D1, Fields{{d->adv, 3}}, kernel, [&](const PhaseMirror& m) -> int {
			HNS_TRY(kernel(d->gO, st));
			return chain_mirror<3>(m, &d->adv, 1);
		});
	}

	// :172-176, out of place (the reference's in-place launch races)
	int vorticity() {
		const float ix = inv_dx();
		HNS_TRY(stencil(PhaseKind::Vorticity, X_D1, Fields{{d->tmp, 3}},
		                [&](hns_grid* g, hipStream_t s) { return hns_dev_vorticity_confinement(g, d->adv, d->tmp, dt, ix, prm->vorticityScale, prm->factorScale, s); }, no_chain));
		std::swap(d->adv, d->tmp);
		return HNS_OK;
	}

	// divergence (:181-188); full: + what combustion adds to it over the same leaves (:211-221, k_combustion_div: fuel and waste only)
	int divergence() {
		const float ix = inv_dx();
		return stencil(PhaseKind::Divergence, X_DIV, Fields{{d->div, 1}}, [&](hns_grid* g, hipStream_t s) -> int {
			HNS_TRY(hns_dev_divergence(g, d->adv, d->div, ix, s));
			const uint64_t first = g->first_active * 512u, n = g->n_active * 512u;
			return full() && n ? hns_combustion_div(d->phi[(size_t)fi[0]] + first, d->phi[(size_t)fi[1]] + first, d->div + first, prm->expansionRate, n, s) : (int)HNS_OK;
		}, [&](const PhaseMirror& m) { return hns_chain_divergence(d->gO, d->adv, d->div, ix, &m, st); });
	}

	// the rest of combustion, buoyancy with the NEW temperature (:226-234), outputs become inputs (:239-246): pointwise, owned voxels
	int combustion() {
		const uint64_t n_owned = (uint64_t)(d->nB + d->nI) * 512u;
		if (n_owned) {
			HNS_TRY(hns_combustion_fields(d->phi[(size_t)fi[0]], d->phi[(size_t)fi[1]], d->phi[(size_t)fi[2]], d->phi[(size_t)fi[3]], d->phi_next[(size_t)fi[0]],
			                              d->phi_next[(size_t)fi[1]], d->phi_next[(size_t)fi[2]], d->phi_next[(size_t)fi[3]], prm->temperatureRelease, n_owned, st));
			HNS_TRY(hns_dev_temperature_buoyancy(d->adv, d->phi_next[(size_t)fi[2]], d->adv, dt, prm->ambientTemp, prm->buoyancyStrength, n_owned, st));
		}
		Fields f;
		for (int c = 0; c < 4; ++c) {
			std::swap(d->phi[(size_t)fi[c]], d->phi_next[(size_t)fi[c]]);
			f.emplace_back(d->phi[(size_t)fi[c]], 1);
		}
		return post(d, X_ADV, f, st, nothing, nothing);  // advect_scalars reads their ghosts; hidden under the pressure solve
	}

	// hns_dist_timing: the pressure loop's bracket opens in its first block and closes in the gradient phase
	int open_timed() {
		if (hipEvent_t* timed = d->solve_ev.current()) HNS_HIP(hipEventRecord(timed[0], st));
		return HNS_OK;
	}

	// one block of up to k sweeps with the halo of p exchanged behind it; all but the last sweep the ghost leaves too
	int sor_block_exchanged(int b) {
		hns_dist* D = d;
		if (b == 0) it = 0, src = d->p_a, dst = d->p_b;  // never warm-started (reference HNanoSolver.cu:113): the first sweep reads no p
		const int n = std::min(d->k, iterations - it);
		// what the previous phase posted: in full in front of the first block (the divergence's ghosts) and wherever this block starts with sweeps over the ghost leaves;
		// between blocks that sweep owned leaves only, the boundary kernel alone (complete_boundary_only)
		// the one launch over all owned leaves that packs its own messages (below) where the owned range is swept in 16^3 blocks and the plan has pack tables for both region types
		const bool unsplit = in_line_rank() && d->pack_ok[X_P] && d->pack_ok[X_D1] && hns_rbgs_block_packable(d->gO);
		const int tail = unsplit ? std::min(n, 2) : ((n >= 2 && split_blocked()) ? 2 : 1);
		if (b == 0 || n > tail || !complete_boundary_only(d, st)) HNS_TRY(complete(d, st));
		if (b == 0) HNS_TRY(open_timed());
		// Round 4: the sweeps of the block that the exchange follows are TWO iterations in one temporally blocked launch per range
		// (hns_sorblock.hip over a launch range: the ghost leaves are tile sources, 2K = 4 voxels deep, and are not swept; the X_P region
		// of a plan with k >= 2 reaches 2k >= 4 voxels, its div region 2k - 1 >= 3), where the library's plan for the ranges says so.
		// With k = 2 that is the whole pressure loop: no sweep ever touches a ghost leaf.
		if (n > tail) {  // the sweeps over owned + ghost leaves as ONE solve of n - tail iterations: the library picks the form (two iterations per launch where that pays)
			int in_b = 0;
			HNS_TRY(hns_rbgs_iterate(d->gA, d->div, src, dst, d->voxel_size, omega_compute(d->voxel_size), n - tail, &in_b, st, it == 0));
			if (in_b) std::swap(src, dst);
			it += n - tail;
		}
		const bool last = it + tail == iterations, zero = it == 0;
		float *s0 = src, *d0 = dst;
		const float vs = d->voxel_size;
		auto part = [=](hns_grid* g, hipStream_t s) {
			return g->n_active ? hns_rbgs_iterate(g, D->div, s0, d0, vs, omega_compute(vs), tail, nullptr, s, zero) : (int)HNS_OK;
		};
		const int xt = last ? X_D1 : X_P;
		auto pack_launch = [=](hns_grid* g, int its, hipStream_t s, bool* done) {  // the blocked sweep that writes the peers' messages as it stores (PackMirror)
			PackMirror m = D->pack_type[xt];
			for (size_t pi = 0; pi < D->peers.size(); ++pi) m.msg[pi] = D->peers[pi].sbuf[D->pending.parity];
			return hns_rbgs_block_pack_launch(g, D->div, s0, d0, vs, omega_compute(vs), zero, &m, s, done, its);
		};
		// Round 6: ONE launch over all owned leaves that packs the peers' messages as it stores (PackMirror), then the transfer and the unpack behind it on the compute stream.
		// The boundary / interior split (below) buys overlap of the transfer with the interior sweep, and pays for it: a 16^3 block that straddles the boundary layer is swept by
		// both launches (config 5, rank 4 of 8: 14 + 14 us against 19 for the one launch), two cross-stream event edges per exchange, and twice the runtime calls -- traced, the
		// split loop's chain boundary sweep -> transfer -> unpack -> next boundary sweep alone took longer than this whole sequence (profiles/r06_dist_exchanged_notes.txt).
		if (unsplit) {
			HNS_TRY(post(d, xt, Fields{{dst, 1}}, st, [=](hipStream_t s) -> int {
				bool done = false;
				HNS_TRY(pack_launch(D->gO, tail, s, &done));
				if (!done) return fail(HNS_ERR_RUNTIME, "hns_dist: the owned range is not swept in 16^3 blocks after all");
				D->pending.prepacked = true;
				return HNS_OK;
			}, nothing, true));
		} else {
			HNS_TRY(post(d, xt, Fields{{dst, 1}}, st, [=](hipStream_t s) -> int {
				// two iterations in one blocked launch: the boundary sweep packs the messages itself
				if (tail == 2 && D->pack_ok[xt]) {
					bool done = false;
					HNS_TRY(pack_launch(D->gB, 2, s, &done));
					if (done) {
						D->pending.prepacked = true;
						return HNS_OK;
					}
				}
				return part(D->gB, s);
			}, [=](hipStream_t s) { return part(D->gI, s); }));
		}
		std::swap(src, dst);
		it += tail;
		if (last) d->p_result = src;
		return HNS_OK;
	}

	// one block of the mirror pressure loop: ONE chained launch of the temporally blocked form, two iterations or the odd one left over (every rank alike: blocked_mirror)
	int mirror_block(int b) {
		if (b == 0) {
			it = 0, src = d->p_a, dst = d->p_b;  // never warm-started (reference HNanoSolver.cu:113): the first sweep reads no p
			HNS_TRY(open_timed());
		}
		const int its = std::min(2, iterations - it);
		const PhaseMirror m = phase_args(d, X_P, Fields{{dst, 1}});
		const bool zero = it == 0;
		HNS_TRY(chained(m, [&] { return hns_rbgs_block_mirror_launch(d->gO, d->div, src, dst, d->voxel_size, omega_compute(d->voxel_size), zero, &m, st, its); }));
		std::swap(src, dst);
		it += its;
		if (it == iterations) d->p_result = src;
		return launch_status("hns_dist: blocked mirror sweep");
	}

	// gradient subtraction (:278-289) [and collision, :292-296] -> u, whose ghosts the scalar advection reads
	int gradient() {
		if (!full() && d->mirror && !d->chain && d->mir.n_peers) {  // the gradient reads what the peers' last sweep wrote into the ghost voxels
			// (here and not behind the last sweep: locally connected ranks share one stream, and a rank's wait must not sit in
			// front of the sweeps it waits for)
			PhaseMirror m = d->mir;
			m.seq = d->sweep_seq;
			hipLaunchKernelGGL(k_sweep_wait, dim3(1), dim3(64), 0, st, m);
		}
		if (hipEvent_t* timed = d->solve_ev.current()) {  // the timed region ends when the last refresh of p has landed (complete() in front of the phase)
			HNS_HIP(hipEventRecord(timed[1], st));
			d->solve_ev.advance();
			d->timed_sweeps += iterations;
		}
		const float ix = inv_dx();
		return stencil(PhaseKind::Gradient, X_ADV, Fields{{d->u, 3}}, [&](hns_grid* g, hipStream_t s) -> int {
			HNS_TRY(hns_dev_subtract_pressure_gradient(g, d->adv, d->p_result, d->u, sdf(), coll ? 1 : 0, ix, s));
			return coll ? hns_dev_enforce_collision_boundaries(g, d->u, sdf(), d->voxel_size, s) : (int)HNS_OK;
		}, [&](const PhaseMirror& m) {  // (its boundary workgroups wait for the peers' last sweep themselves)
			return hns_chain_subtract_pressure_gradient(d->gO, d->adv, d->p_result, d->u, ix, &m, st);
		});
	}

	// advect every float field except collision_sdf with the projected velocity (:321-356), and already post them for the advection that opens the next substep
	int advect_scalars() {
		d->u_ghosts_fresh = !coll;  // (with collision the next substep rewrites u before it advects)
		const float ix = inv_dx();
		std::vector<const float*> in;
		std::vector<float*> out;
		std::vector<int> which;
		for (int s = 0; s < d->n_scalars; ++s)
			if (s != fi[4]) in.push_back(d->phi[(size_t)s]), out.push_back(d->phi_next[(size_t)s]), which.push_back(s);
		const int ns = (int)in.size();
		if (ns) {
			Fields f;
			for (float* p : out) f.emplace_back(p, 1);  // the boundary leaves' new values travel while the interior is advected
			auto kernel = [&](hns_grid* g, hipStream_t s) {
				return g->n_active ? hns_dev_advect_scalars(g, d->u, in.data(), out.data(), ns, sdf(), coll ? 1 : 0, dt, ix, s) : (int)HNS_OK;
			};
			HNS_TRY(stencil(PhaseKind::AdvectScalars, X_ADV, std::move(f), kernel, [&](const PhaseMirror& m) -> int {
				HNS_TRY(kernel(d->gO, st));
				return chain_mirror<1>(m, out.data(), ns);
			}));
		}
		for (int s : which) std::swap(d->phi[(size_t)s], d->phi_next[(size_t)s]);
		// (chained: the peers' ghost copies of phi are already being written, nothing to open the next substep with -- whether or not the rank has scalars)
		d->phi_in_flight = chained_form() || (ns > 0 && d->world > 1);
		return HNS_OK;
	}
};

// ---- the whole Compute_Sim substep, partitioned (reference HNanoSolver.cu:150-356; single GPU: hns_sim_substep) ----
// field_index: positions of fuel, waste, temperature, flame and collision_sdf (-1: none) among the rank's scalars (hns_dist_upload
// order). Every float field except collision_sdf is advected. Owned results equal hns_sim_substep's on the whole domain bit for bit.
struct SimArgs { const hns_combustion_params* params; const int* field_index; int has_collision; };

int sim_step_args(const hns_dist* d, const SimArgs& a, Step& s) {
	const int* field_index = a.field_index;
	if (!a.params || !field_index) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_sim_substep: null argument");
	for (int c = 0; c < 4; ++c) {
		if (field_index[c] < 0 || field_index[c] >= d->n_scalars) {
			set_error("Missing required input field for combustion: %s", kCombustionFields[c]);  // HNanoSolver.cu:193-201
			return HNS_ERR_RUNTIME;
		}
		for (int e = 0; e < c; ++e)
			if (field_index[e] == field_index[c]) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_sim_substep: two combustion fields share one scalar");
	}
	if (field_index[4] >= d->n_scalars) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_sim_substep: collision_sdf index out of range");
	for (int c = 0; c < 4; ++c)
		if (field_index[4] >= 0 && field_index[4] == field_index[c]) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_sim_substep: collision_sdf shares a scalar with a combustion field");
	// vorticity confinement reads u* up to (int)factor_scale + 1 voxels from a voxel: it must stay inside the one-leaf ghost layer
	if ((int)a.params->factorScale > 6 || (int)a.params->factorScale < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_sim_substep: factor_scale must be within 0..6 on a partitioned domain");
	s.prm = a.params;
	for (int c = 0; c < 5; ++c) s.fi[c] = field_index[c];
	s.coll = a.has_collision && field_index[4] >= 0;  // HNanoSolver.cu:66-75 (collision_sdf itself is never advected, used or not: :327)
	s.vort = (int)a.params->factorScale != 0;  // (int)factor_scale == 0: the kernel is a bit-exact copy (hns_api.hip: Substep::part_a)
	return HNS_OK;
}

// The names of an entry point pair: a rank stepped on its own, and ranks connected with hns_dist_connect_local stepped together.
struct EntryPoint { const char *single, *local; };
constexpr EntryPoint kCore{"hns_dist_core_substep", "hns_dist_local_core_substep"}, kSim{"hns_dist_sim_substep", "hns_dist_local_sim_substep"};

// The preamble of every entry point, for one rank: its checks (`local_world` > 0: one of that many locally connected ranks; 0: a rank on its own), then
// the statistics of the last substep are cleared and the rank's Step is set up (`sim`: the full substep; null: the core).
int begin_rank(hns_dist* d, int iterations, float dt, void* stream, const EntryPoint& e, int local_world, const SimArgs* sim, std::vector<Step>& steps) {
	if (!d) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_core_substep: null handle");
	if (dt < 0.0f) return fail(HNS_ERR_INVALID_ARGUMENT, "dt (time step) cannot be negative.");
	if (iterations <= 0) return fail(HNS_ERR_INVALID_ARGUMENT, "Number of pressure iterations must be positive.");
	HNS_TRY(far_check(d));  // (raised by an earlier substep: kernels are asynchronous; hns_dist_synchronize / hns_dist_download report it too)
	if (local_world) {
		if ((int)d->local_ranks.size() != local_world) return fail(HNS_ERR_INVALID_ARGUMENT, (std::string(e.local) + ": ranks are not locally connected").c_str());
	} else {
		if (!d->gA) return fail(HNS_ERR_NO_DEVICE, (std::string(e.single) + ": plan-only handle (there is no CPU fallback)").c_str());
		if (!d->local_ranks.empty() && d->world > 1) return fail(HNS_ERR_INVALID_ARGUMENT, (std::string(e.single) + ": locally connected ranks step together (" + e.local + ")").c_str());
		if (d->ipc_status && *(volatile int*)d->ipc_status) return fail(HNS_ERR_RUNTIME, "hns_dist: a peer did not answer within 20 s (one-sided transport); results are invalid");
	}
	memset(d->bytes_sent, 0, sizeof(d->bytes_sent));
	d->messages_sent = d->exchanges = d->packed_exchanges = 0;
	steps.push_back(Step{d, iterations, dt, (hipStream_t)stream});
	return sim ? sim_step_args(d, *sim, steps.back()) : (int)HNS_OK;
}

// One rank on its own (RCCL, ipc or loopback transport, or world == 1), asynchronous on `stream` (plus the rank's communication stream).
int substep(hns_dist* d, int iterations, float dt, void* stream, const EntryPoint& e, const SimArgs* sim) {
	std::vector<Step> steps;
	HNS_TRY(begin_rank(d, iterations, dt, stream, e, 0, sim, steps));
	for (const Phase& p : steps[0].phases()) HNS_TRY(steps[0].run(p));
	return HNS_OK;
}

// Ranks connected with hns_dist_connect_local advance in lock step, phase by phase on `stream`: a message may be the sender's field itself (whole-leaf
// regions are not packed), so every rank takes delivery of the previous phase's exchange before any rank's next kernel overwrites what was sent.
// `complete_before_open`: the same in front of phase 0 (the full substep; see hns_dist_local_sim_substep).
int local_substep(hns_dist* const* ranks, int world, int iterations, float dt, void* stream, const EntryPoint& e, const SimArgs* sim, bool complete_before_open) {
	if (!ranks || world < 1) return fail(HNS_ERR_INVALID_ARGUMENT, (std::string(e.local) + ": bad arguments").c_str());
	std::vector<Step> steps;
	for (int r = 0; r < world; ++r) HNS_TRY(begin_rank(ranks[r], iterations, dt, stream, e, world, sim, steps));
	// every rank runs rank 0's list: ranks whose lists differ (created with different sweeps_per_exchange: hns_dist_connect_local does not compare it) are refused here
	const std::vector<Phase> phases = steps[0].phases();
	for (const Step& s : steps)
		if (s.phases() != phases) return fail(HNS_ERR_INVALID_ARGUMENT, (std::string(e.local) + ": ranks with different phases (created with different sweeps_per_exchange?)").c_str());
	for (size_t i = 0; i < phases.size(); ++i) {
		if (i > 0 || complete_before_open)
			for (Step& s : steps) HNS_TRY(complete(s.d, s.st));
		for (Step& s : steps) HNS_TRY(s.run(phases[i]));
	}
	return HNS_OK;
}

}  // namespace

extern "C" {

// One core substep (advect_vector -> divergence -> iterations x RB-SOR -> gradient subtraction -> advect_scalars) of this
// rank, asynchronous on `stream` (plus the rank's communication stream). RCCL transport, or world == 1.
int hns_dist_core_substep(hns_dist* d, int iterations, float dt, void* stream) { return substep(d, iterations, dt, stream, kCore, nullptr); }

// The same for ranks connected with hns_dist_connect_local: all ranks advance phase by phase on `stream`.
int hns_dist_local_core_substep(hns_dist* const* ranks, int world, int iterations, float dt, void* stream) {
	return local_substep(ranks, world, iterations, dt, stream, kCore, nullptr, false);
}

// the whole Compute_Sim substep, partitioned (see SimArgs)
int hns_dist_sim_substep(hns_dist* d, int iterations, float dt, const hns_combustion_params* params, const int* field_index, int has_collision, void* stream) {
	const SimArgs a{params, field_index, has_collision};
	return substep(d, iterations, dt, stream, kSim, &a);
}

// (complete before phase 0 too: with collision that phase rewrites u and posts it again, and a rank must have taken delivery of the exchange the
// previous substep left in flight before a peer posts the next one)
int hns_dist_local_sim_substep(hns_dist* const* ranks, int world, int iterations, float dt, const hns_combustion_params* params, const int* field_index, int has_collision,
                               void* stream) {
	const SimArgs a{params, field_index, has_collision};
	return local_substep(ranks, world, iterations, dt, stream, kSim, &a, true);
}

int hns_dist_timing(hns_dist* d, int max_solves) {
	if (!d || max_solves < 0) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_timing: bad arguments");
	d->timed_sweeps = 0;
	return d->solve_ev.reset(max_solves);
}

int hns_dist_pressure_time(hns_dist* d, float* total_ms, long long* sweeps) {
	if (!d || !total_ms || !sweeps) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_pressure_time: null argument");
	double tot;
	HNS_TRY(d->solve_ev.elapsed(&tot));
	*total_ms = (float)tot;
	*sweeps = d->timed_sweeps;
	return HNS_OK;
}

int hns_dist_synchronize(hns_dist* d, void* stream) {
	if (!d) return fail(HNS_ERR_INVALID_ARGUMENT, "hns_dist_synchronize: null handle");
	HNS_HIP(hipStreamSynchronize((hipStream_t)stream));
	if (d->cs) HNS_HIP(hipStreamSynchronize(d->cs));
	if (d->ipc_status && *(volatile int*)d->ipc_status) return fail(HNS_ERR_RUNTIME, "hns_dist: a peer did not answer within 20 s (one-sided transport); results are invalid");
	return far_check(d);
}

}  // extern "C"
