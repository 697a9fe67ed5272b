// pg_kernels_filter.hip -- recording into sdTree_current through the training filters of pg_set_splat_filter
// (include/pgsd.h states the semantics; this file follows them operation by operation):
//   stochastic box in space : the record's position is jittered by the extent of its KD leaf before the leaf is looked up;
//   overlap box in space    : the record is shared between all KD leaves that a box the size of its KD leaf, placed around its
//                             position and shifted to stay inside the root box, overlaps, each in proportion to the overlap's
//                             volume;
//   box in direction        : a (direction, weight) pair is shared between all quadtree leaves that a square the size of its
//                             nearest leaf, centred on the direction, overlaps.
// Accumulators exist at quadtree leaves only and all sums are integers (pg_kernels_splat.hip), so a filtered record is just
// more integer adds, and they leave through the same coop_add.  A pair makes 1 to dozens of deposits, so the lanes of a wave
// do not finish together, and an atomic between two gathers makes the second gather wait for it (the memory counter of a wave
// returns in order).  The walks therefore only QUEUE their deposits -- 8 bytes each, in a ring of the wave's own LDS -- in rounds
// that go on while any lane still has a part; the queue is drained by full waves, one cooperative add per 64 deposits, when it
// is nearly full and at the end.
//
// The footprint meets at most a 2 x 2 block of cells of the nearest leaf's depth d, but below such a cell there may be a subtree
// of finer leaves of any depth.  Its leaves are enumerated WITHOUT a stack (a per-lane array indexed by the level would be
// scratch memory): the walk keeps the record of the depth-d cell (the anchor), the level it stands on and the child it stands
// at on every level above -- two bits per level in one 64-bit word -- and, when it has finished a record's four children,
// climbs by walking down again from the anchor along those bits.  Subtrees the footprint does not reach are never entered.
// The KD leaves under a record's box are enumerated the same way (KdWalk), one bit per level.
#include "pg_descent.hpp"
#include "pg_kernels.hpp"
#include "pg_splat_dev.hpp"

namespace pg {

// the four child words of a record (0 = that child is a leaf)
__device__ __forceinline__ uint4 load_children(const QuadRec *rec, uint32_t r)
{
	return gather16(reinterpret_cast<const uint4 *>(rec + r) + 1);
}

// child number of the quadrant (x high?, y high?): 0 -> (1, 1), 1 -> (0, 1), 2 -> (0, 0), 3 -> (1, 0) (quadtree.py:153-175)
__device__ __forceinline__ uint32_t child_of(uint32_t xh, uint32_t yh) { return yh ? (xh ? 0u : 1u) : (xh ? 3u : 2u); }

__device__ __forceinline__ float pow2_neg(uint32_t k) { return __uint_as_float((127u - k) << 23); } // 2^-k, k <= 126

// One (direction, weight) pair on its way into the tree: what is still to be added.
struct BoxWalk {
	bool active;        // parts are left
	bool box;           // the footprint is being enumerated (else: one nearest deposit)
	uint32_t nidx;      // accumulator of the nearest leaf N (receives the record count)
	long long count;    // 1: the record counts (inside the root box, path direction), not delivered yet
	float w;
	uint32_t tree, d;   // the quadtree; depth of N
	float tx, ty;       // include/pgsd.h: the footprint's offset in cells of depth d
	uint32_t X0, Y0;
	uint32_t q;         // next cell of the 2 x 2 block to open: a = q & 1, b = q >> 1; 4: none left
	// the open cell's subtree
	uint32_t anchor;    // record of the open depth-d cell, kNoRecord: no cell is open
	uint32_t k;         // level below the anchor the walk stands on (0: the anchor's own children)
	uint64_t path;      // child the walk stands at on level l: bits 2l, 2l + 1
	uint32_t r;         // record on level k
	uint4 ch;           // its child words
	float ulo, vlo;     // its cell's corner in the open cell's frame
	float lx, hx, ly, hy; // the footprint in the open cell's frame
	bool restart;       // r / ch / ulo / vlo have to be walked down again from the anchor
};

// A deposit on its way to its accumulator.  Accumulators are numbered through the one buffer [rec_acc | root_acc]
// (pg_tree.hpp): slot rec * 4 + child, and n_rec * 4 + tree for the root accumulator of a tree whose root is a leaf.
constexpr uint32_t kNoPart = 0xffffffffu;
constexpr uint32_t kPartCount = 0x80000000u; // bit 31 of a queued index: the deposit carries the record's count
struct Part {
	uint32_t idx; // accumulator, kNoPart: nothing
	float p;      // the weight to quantise
	bool count;
};

// starts the deposits of one pair whose nearest walk has finished in `c`
__device__ __forceinline__ void box_begin(BoxWalk &b, const TreeView &t, uint32_t tree, const LeafCursor &c, float w,
                                          long long count, bool directional_box)
{
	b.active = c.found;
	b.box = false;
	b.nidx = kNoPart;
	b.count = count;
	b.w = w;
	b.tree = tree;
	b.q = 4;
	b.anchor = kNoRecord;
	if (!c.found) return;
	b.nidx = c.is_root ? t.n_rec * 4u + tree : c.slot;
	b.d = stat_levels(c.levels);
	// (a root leaf, or a weight every part of which truncates to nothing: the nearest deposit is the whole of it)
	// (d <= 30: the depth limit of pg_setup and pg_import)
	if (!directional_box || c.is_root || b.d == 0 || b.d > 30u || quantize_weight(w).zero()) return;
	b.box = true;
	const float G = (float)(1u << b.d);
	const float vx = c.cx * G - 0.5f;
	const float fjx = __builtin_floorf(vx);
	b.tx = vx - fjx;
	b.X0 = (uint32_t)(int32_t)fjx & ((1u << b.d) - 1u);
	float vy = c.cy * G - 0.5f;
	vy = vy > 0.0f ? vy : 0.0f;
	const float fjy = __builtin_floorf(vy);
	b.ty = vy - fjy;
	uint32_t jy = (uint32_t)(int32_t)fjy;
	if (jy >= (1u << b.d) - 1u) { jy = (1u << b.d) - 1u; b.ty = 0.0f; }
	b.Y0 = jy;
	b.q = 0;
}

// The next deposit of the pair, or one without a target when this call found none (the caller goes on calling while
// b.active).  The work of one call is bounded, so that the lanes of a wave come back to the cooperative add together often.
__device__ __forceinline__ Part box_next(BoxWalk &b, const TreeView &t, const TreeHead &head)
{
	const Part none = {kNoPart, 0.0f, false};
	if (!b.active) return none;
	if (!b.box) { // nearest: one deposit, with the count
		b.active = false;
		const Part s = {b.nidx, b.w, b.count != 0};
		return s;
	}
	const uint32_t d = b.d, Gm = (1u << d) - 1u;
	for (int guard = 0; guard < 8; ++guard) { // (bounded work per call)
		if (b.anchor == kNoRecord) {
			if (b.q >= 4) { // every cell done: the count, should no deposit have carried it (it always has, but for roundings at depths > 23)
				b.active = false;
				if (b.count == 0) return none;
				const Part s = {b.nidx, 0.0f, true};
				b.count = 0;
				return s;
			}
			const uint32_t qa = b.q & 1u, qb = b.q >> 1;
			++b.q;
			const float ax0 = 1.0f - b.tx, ay0 = 1.0f - b.ty;          // widths of column 0 / row 0; column 1 / row 1: tx, ty
			const float fa = qa ? b.tx : ax0, fb = qb ? b.ty : ay0;
			if (!(fa > 0.0f && fb > 0.0f)) continue;                    // an empty column or row
			const bool other_col = (qa ? ax0 : b.tx) > 0.0f, other_row = (qb ? ay0 : b.ty) > 0.0f;
			const uint32_t X1 = (b.X0 + 1u) & Gm, Y1 = b.Y0 + 1u;
			const uint32_t X = qa ? X1 : b.X0, Y = qb ? Y1 : b.Y0;
			// the node of cell (X, Y) at depth d: through the jump table where it leads there, else from the root
			uint32_t r = head.root_rec, L = 0, leaf_slot = kSlotNone;
			if (t.jump.p != nullptr) {
				const int bits = t.jump.bits;
				const uint32_t jx = (int)d >= bits ? X >> (d - bits) : X << (bits - d);
				const uint32_t jy = (int)d >= bits ? Y >> (d - bits) : Y << (bits - d);
				const uint4 e = gather16(t.jump.p + (((size_t)b.tree << (2 * bits)) + ((jy << bits) | jx)));
				const uint32_t Lj = (e.w >> 26) & 15u;
				if (Lj <= d && (e.w >> 31) == 0u) {
					L = Lj;
					if (e.x == kNoRecord) leaf_slot = e.w & kJumpSlotMask;
					else r = e.x;
				}
			}
			while (leaf_slot == kSlotNone && L < d) {
				const uint4 ch = load_children(t.rec, r);
				const uint32_t bit = d - 1u - L;
				const uint32_t j = child_of((X >> bit) & 1u, (Y >> bit) & 1u);
				const uint32_t c = sel4u((int)j, ch.x, ch.y, ch.z, ch.w);
				++L;
				if (c == 0) leaf_slot = r * 4u + j;
				else r = c;
			}
			if (leaf_slot != kSlotNone) { // a leaf at depth L <= d that holds the cell -- and perhaps its neighbours in the block
				const uint32_t sh = d - L;
				const bool col_merge = other_col && (b.X0 >> sh) == (X1 >> sh);
				const bool row_merge = other_row && (b.Y0 >> sh) == (Y1 >> sh);
				if ((qa && col_merge) || (qb && row_merge)) continue;   // deposited when its first cell was opened
				const float ox = col_merge ? 1.0f : fa, oy = row_merge ? 1.0f : fb;
				Part s = {leaf_slot, b.w * (ox * oy), false};
				if (leaf_slot == b.nidx) { s.count = b.count != 0; b.count = 0; }
				return s;
			}
			// the cell is subdivided: walk its subtree
			b.anchor = r;
			b.k = 0;
			b.path = 0;
			b.r = r;
			b.ch = load_children(t.rec, r);
			b.ulo = 0.0f; b.vlo = 0.0f;
			b.lx = qa ? 0.0f : b.tx; b.hx = qa ? b.tx : 1.0f;
			b.ly = qb ? 0.0f : b.ty; b.hy = qb ? b.ty : 1.0f;
			b.restart = false;
			continue;
		}
		if (b.restart) { // back on level k: down again from the anchor
			uint32_t r = b.anchor;
			float ulo = 0.0f, vlo = 0.0f;
			for (uint32_t l = 0; l < b.k; ++l) {
				const uint4 ch = load_children(t.rec, r);
				const uint32_t j = (uint32_t)(b.path >> (2u * l)) & 3u;
				const float h = pow2_neg(l + 1u);
				if (j == 0u || j == 3u) ulo += h;
				if (j == 0u || j == 1u) vlo += h;
				r = sel4u((int)j, ch.x, ch.y, ch.z, ch.w);
			}
			b.r = r;
			b.ch = load_children(t.rec, r);
			b.ulo = ulo; b.vlo = vlo;
			b.restart = false;
		}
		// the child the walk stands at
		const uint32_t j = (uint32_t)(b.path >> (2u * b.k)) & 3u;
		const float h = pow2_neg(b.k + 1u);
		const float u0 = (j == 0u || j == 3u) ? b.ulo + h : b.ulo, v0 = (j == 0u || j == 1u) ? b.vlo + h : b.vlo;
		const float u1 = u0 + h, v1 = v0 + h;
		const float ox = (u1 < b.hx ? u1 : b.hx) - (u0 > b.lx ? u0 : b.lx);
		const float oy = (v1 < b.hy ? v1 : b.hy) - (v0 > b.ly ? v0 : b.ly);
		const uint32_t c = sel4u((int)j, b.ch.x, b.ch.y, b.ch.z, b.ch.w);
		const bool hit = ox > 0.0f && oy > 0.0f;
		if (hit && c != 0 && b.k + 1u < (uint32_t)kMaxLevels) { // an inner node the footprint reaches: down
			++b.k;
			b.path &= ~(3ull << (2u * b.k));
			b.r = c;
			b.ch = load_children(t.rec, c);
			b.ulo = u0; b.vlo = v0;
			continue;
		}
		Part s = none;
		if (hit && c == 0) {
			s.idx = b.r * 4u + j;
			s.p = b.w * (ox * oy);
			if (s.idx == b.nidx) { s.count = b.count != 0; b.count = 0; }
		}
		// on to the next child; a record whose four children are done hands back to its parent
		uint32_t k = b.k;
		for (;;) {
			const uint32_t dj = (uint32_t)(b.path >> (2u * k)) & 3u;
			if (dj < 3u) { b.path += 1ull << (2u * k); break; }
			b.path &= ~(3ull << (2u * k));
			if (k == 0) { b.anchor = kNoRecord; break; }
			--k;
			b.restart = true;
		}
		b.k = k;
		if (s.idx != kNoPart) return s;
	}
	return none;
}

// what the KD part of a filtered record yields: the quadtree and whether the record counts
struct KdPlan {
	uint32_t tree;
	bool inside;
};

// KDTree.addDataPropagate's leaf lookup (kdtree.py:180-225) behind the spatial filter
__device__ __forceinline__ KdPlan plan_kd(const TreeView &t, const float *planes, const pg_filter_args &f, uint32_t index,
                                          float x, float y, float z)
{
	KdPlan p;
	p.inside = inside_root(t, x, y, z);
	KdNode leaf;
	uint32_t lv;
	if (f.spatial && p.inside) {
		const uint32_t node = kd_descend_grid(t, planes, x, y, z, true, leaf, lv);
		const float *lo = f.kd_bmin + 3 * (size_t)node, *hi = f.kd_bmax + 3 * (size_t)node;
		Pcg32 rng = pcg32_seed(f.seed, index);
		float q[3] = {x, y, z};
#pragma unroll
		for (int a = 0; a < 3; ++a) {
			const float e = hi[a] - lo[a];
			const float u = rng.next_f32();
			float v = q[a] + (u - 0.5f) * e;
			v = v > t.bmin[a] ? v : t.bmin[a];
			v = v < t.bmax[a] ? v : t.bmax[a];
			q[a] = v;
		}
		x = q[0]; y = q[1]; z = q[2];
	}
	kd_descend_grid(t, planes, x, y, z, p.inside, leaf, lv);
	p.tree = leaf.tree; // outside the bbox: node 0's (stale) tree (kdtree.py:224)
	return p;
}

// ---- PG_SPATIAL_OVERLAP_BOX: the KD leaves under a record's box ----
__device__ __forceinline__ float sel3f(uint32_t k, float a, float b, float c) { return k == 0u ? a : (k == 1u ? b : c); }
__device__ __forceinline__ float minf(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float maxf(float a, float b) { return a > b ? a : b; }

// The depth-first walk over the KD leaves a box reaches, WITHOUT a stack: the child taken on every level (`path`, one bit per
// level) and the levels on which the right child is still to be visited (`pend`).  A finished leaf hands over to the right
// child of the deepest pending level: the walk goes down again along `path` -- from the anchor, the node at which it first
// had to go both ways while nothing was pending: everything still to be visited lies below it.
struct KdWalk {
	bool active;
	uint32_t home;            // L, the leaf of the record's own position: the caller has dealt with it
	float lx, ly, lz, hx, hy, hz; // the box
	float ex, ey, ez;         // its extent: that of L
	uint32_t node, k;         // the node the walk stands on and its level
	uint32_t child, axis;     // its child word (0: a leaf) and split axis
	float split;
	uint32_t tree;            // a leaf's quadtree
	uint32_t path, pend, fk;  // below level fk the walk follows `path` instead of deciding
	uint32_t anchor, anchor_k;
};

__device__ __forceinline__ void kd_walk_load(KdWalk &w, const TreeView &t, uint32_t node)
{
	const KdNode nd = load_kd(t.kd, node);
	w.node = node;
	w.child = nd.child;
	w.axis = nd.axis_depth & 3u;
	w.split = nd.split;
	w.tree = nd.tree;
}

// include/pgsd.h: the share of KD node `node` in the box of `w`; false: it takes no part
__device__ __forceinline__ bool kd_share(const KdWalk &w, const pg_filter_args &f, uint32_t node, float &s)
{
	const float *lo = f.kd_bmin + 3 * (size_t)node, *hi = f.kd_bmax + 3 * (size_t)node;
	const float l0 = minf(hi[0], w.hx) - maxf(lo[0], w.lx);
	const float l1 = minf(hi[1], w.hy) - maxf(lo[1], w.ly);
	const float l2 = minf(hi[2], w.hz) - maxf(lo[2], w.lz);
	s = ((l0 / w.ex) * (l1 / w.ey)) * (l2 / w.ez);
	return l0 > 0.0f && l1 > 0.0f && l2 > 0.0f;
}

// The record's box, and the walk over it made ready at the root.  False: the record is handled as PG_SPATIAL_NEAREST (L is the
// root, or an extent of L is not a positive finite number).
__device__ __forceinline__ bool kd_walk_begin(KdWalk &w, const TreeView &t, const pg_filter_args &f, uint32_t L, float x, float y,
                                              float z)
{
	w.active = false;
	w.home = L;
	if (L == 0u) return false;
	const float *lo = f.kd_bmin + 3 * (size_t)L, *hi = f.kd_bmax + 3 * (size_t)L;
	const float p[3] = {x, y, z};
	float e[3], bl[3], bh[3];
	bool ok = true;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		e[a] = hi[a] - lo[a];
		ok = ok && e[a] > 0.0f && e[a] < __builtin_inff(); // (NaN fails both)
		bl[a] = maxf(p[a] - 0.5f * e[a], t.bmin[a]);
		bh[a] = bl[a] + e[a];
		if (bh[a] > t.bmax[a]) { bh[a] = t.bmax[a]; bl[a] = maxf(bh[a] - e[a], t.bmin[a]); }
	}
	if (!ok) return false;
	w.ex = e[0]; w.ey = e[1]; w.ez = e[2];
	w.lx = bl[0]; w.ly = bl[1]; w.lz = bl[2];
	w.hx = bh[0]; w.hy = bh[1]; w.hz = bh[2];
	w.k = 0; w.path = 0; w.pend = 0; w.fk = 0;
	w.anchor = 0; w.anchor_k = 0;
	kd_walk_load(w, t, 0u);
	w.active = true;
	return true;
}

// The next KD leaf other than L that takes part, with its quadtree and share -- or false when this call found none (the caller
// goes on calling while w.active).  The work of one call is bounded, like box_next's.
__device__ __forceinline__ bool kd_walk_next(KdWalk &w, const TreeView &t, const pg_filter_args &f, uint32_t &tree, float &s)
{
	for (int guard = 0; guard < 8 && w.active; ++guard) {
		if (w.child != 0u && w.k < 31u) { // an inner node: down (KD depth <= 30: the depth limit of pg_setup and pg_import)
			uint32_t bit = (w.path >> w.k) & 1u;
			bool down = true;
			if (w.k >= w.fk) { // a child is visited only if the box reaches across the split plane
				const bool left = sel3f(w.axis, w.lx, w.ly, w.lz) < w.split, right = sel3f(w.axis, w.hx, w.hy, w.hz) > w.split;
				bit = left ? 0u : 1u;
				down = left || right;
				if (left && right) {
					if (w.pend == 0u) { w.anchor = w.node; w.anchor_k = w.k; }
					w.pend |= 1u << w.k;
				}
				w.path = (w.path & ~(1u << w.k)) | (bit << w.k);
			}
			if (down) {
				kd_walk_load(w, t, w.child + bit);
				++w.k;
				continue;
			}
		}
		bool found = false;
		if (w.child == 0u && w.node != w.home) {
			found = kd_share(w, f, w.node, s);
			tree = w.tree;
		}
		if (w.pend == 0u) w.active = false;
		else { // on to the right child of the deepest pending level
			const uint32_t l = 31u - (uint32_t)__builtin_clz(w.pend);
			w.pend &= ~(1u << l);
			w.path = (w.path & ((1u << l) - 1u)) | (1u << l);
			w.fk = l + 1u;
			if (w.k == l + 1u) kd_walk_load(w, t, w.node + 1u); // the walk stands on its left child: the children of a node are adjacent
			else {
				w.k = w.anchor_k;
				kd_walk_load(w, t, w.anchor);
			}
		}
		if (found) return true;
	}
	return false;
}

// The wave's queue of deposits: kQueue entries of {accumulator | count flag, weight} in LDS, filled by the walks' rounds and
// drained 64 at a time through coop_add.  `len` is uniform over the wave.
constexpr uint32_t kQueue = 512;
static_assert(kQueue >= 128, "a round appends up to 64 entries to a queue that is drained above kQueue - 64");

__device__ __forceinline__ void queue_drain(const AccumView &a, uint2 *s_q, uint32_t &len, long long *s_val, unsigned long long *s_ptr)
{
	const uint32_t lane = threadIdx.x & 63u;
	wave_lds_sync(); // the appends are visible
	for (uint32_t head = 0; head < len; head += 64u) {
		SlotAdd s = {nullptr, 0, 0, 0, 0};
		if (head + lane < len) {
			const uint2 e = s_q[head + lane];
			const Limbs q = quantize_weight(__uint_as_float(e.y));
			s.ptr = a.rec_acc + (size_t)kAccWords * (e.x & ~kPartCount);
			s.w0 = q.l0; s.w1 = q.l1; s.w2 = q.l2; s.w3 = (e.x & kPartCount) ? 1 : 0;
		}
		coop_add(s, s_val, s_ptr);
	}
	wave_lds_sync(); // the reads are done before the next append
	len = 0;
}

// The pairs of a record enter quadtree `tree`: the two nearest walks, and the deposits of the path pair (weight w) begun; the
// emitter pair waits in `cn`.  counted: the record's count goes to this tree (and, should its direction reach no leaf, to the
// tree's fallback counter).
__device__ __forceinline__ void open_tree(const TreeView &t, const AccumView &a, const pg_filter_args &f, int store_nee, uint32_t tree,
                                          bool counted, float dx, float dy, float nx, float ny, float w, BoxWalk &b, TreeHead &head,
                                          LeafCursor &cn, bool &second)
{
	head = load_head_s(t.head, tree);
	const JumpPre pre_p = jump_prefetch(t.jump, tree, dx, dy, in_unit_square(dx, dy));
	const JumpPre pre_n = jump_prefetch(t.jump, tree, nx, ny, store_nee != 0 && in_unit_square(nx, ny));
	LeafCursor cp = leaf_cursor_pre(head, dx, dy, true, pre_p);
	cn = leaf_cursor_pre(head, nx, ny, store_nee != 0, pre_n);
	quad_find_leaf_slots2(t.rec, cp, cn);
	// a counted record whose direction reaches no leaf (outside the unit square): fallback counter
	if (counted && !cp.found) atomicAdd(a.leaf_count + tree, 1ull);
	box_begin(b, t, tree, cp, w, counted ? 1 : 0, f.directional != 0);
	second = store_nee != 0 && cn.found;
}

// One record: the KD leaf (jittered or not) -- kOverlap: one KD leaf under the record's box after the other, L first --, the
// two nearest walks, then the deposits of both pairs, queued in rounds in which every lane of the wave takes part.
template <bool kOverlap>
__device__ __forceinline__ void splat_filtered(const TreeView &t, const AccumView &a, const float *planes, const pg_filter_args &f,
                                               int store_nee, bool valid, uint32_t index, float x, float y, float z, float dx,
                                               float dy, float radiance, float wo_pdf, float nx, float ny, float nee_lum,
                                               uint2 *s_q, uint32_t &len, long long *s_val, unsigned long long *s_ptr)
{
	BoxWalk b;
	b.active = false;
	b.box = false;
	b.anchor = kNoRecord;
	b.q = 4;
	TreeHead head = {kNoRecord, 0.0f};
	LeafCursor cn;
	cn.found = false;
	float wn = 0.0f;
	uint32_t tree = 0;
	bool second = false; // the emitter pair is still to come
	KdWalk kw;           // (kOverlap) the KD leaves other than L
	kw.active = false;
	float w0 = 0.0f, wn0 = 0.0f; // (kOverlap) the pairs' whole weights
	if (valid) {
		const float w = wo_pdf > 0.0f ? radiance / wo_pdf : 0.0f;   // quadtree.py:451
		wn = wo_pdf > 0.0f ? nee_lum / wo_pdf : 0.0f;               // quadtree.py:462
		if (!kOverlap) {
			const KdPlan kp = plan_kd(t, planes, f, index, x, y, z);
			tree = kp.tree;
			open_tree(t, a, f, store_nee, tree, kp.inside, dx, dy, nx, ny, w, b, head, cn, second);
		} else {
			const bool inside = inside_root(t, x, y, z);
			KdNode leaf;
			uint32_t lv;
			const uint32_t L = kd_descend_grid(t, planes, x, y, z, inside, leaf, lv);
			tree = leaf.tree; // outside the bbox: node 0's (stale) tree (kdtree.py:224)
			w0 = w; wn0 = wn;
			float wl = w;
			if (inside && kd_walk_begin(kw, t, f, L, x, y, z)) { // L's own share; its count does not depend on it
				float s;
				const bool part = kd_share(kw, f, L, s);
				wl = part ? w0 * s : 0.0f;
				wn = part ? wn0 * s : 0.0f;
				// (a record neither direction of which reaches a leaf deposits nothing in any KD leaf)
				kw.active = in_unit_square(dx, dy) || (store_nee != 0 && in_unit_square(nx, ny));
			}
			open_tree(t, a, f, store_nee, tree, inside, dx, dy, nx, ny, wl, b, head, cn, second);
		}
	}
	for (;;) {
		if (!b.active && second) {
			box_begin(b, t, tree, cn, wn, 0, f.directional != 0);
			second = false;
		}
		if (kOverlap && !b.active && kw.active) { // (second is false here: a waiting emitter pair has just made b active)
			float s;
			if (kd_walk_next(kw, t, f, tree, s)) {
				wn = wn0 * s;
				open_tree(t, a, f, store_nee, tree, false, dx, dy, nx, ny, w0 * s, b, head, cn, second);
			}
		}
		// (second: a leaf just opened for the emitter pair alone)
		if (__ballot(b.active || (kOverlap && (second || kw.active))) == 0ull) break;
		const Part s = box_next(b, t, head);
		const bool has = s.idx != kNoPart;
		const unsigned long long m = __ballot(has);
		if (has) {
			const uint32_t pos = len + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
			s_q[pos] = make_uint2(s.idx | (s.count ? kPartCount : 0u), __float_as_uint(s.p));
		}
		len += (uint32_t)__popcll(m);
		if (len > kQueue - 64u) queue_drain(a, s_q, len, s_val, s_ptr);
	}
}

// A filtered kernel's LDS -- the staged KD planes, coop_add's exchange buffers, the waves' queues -- and the state of its
// wave's own queue, which lives across the tiles of a strided kernel
#define PG_FILTER_LDS()                                  \
	__shared__ float s_planes[3 * kKdGridPlanes];        \
	__shared__ long long s_val[kBlock * 4];              \
	__shared__ unsigned long long s_ptr[kBlock];         \
	__shared__ uint2 s_queue[(kBlock / 64) * kQueue];    \
	uint2 *s_q = s_queue + (threadIdx.x >> 6) * kQueue;  \
	uint32_t len = 0

template <bool kOverlap>
__global__ __launch_bounds__(kBlock) void k_filter_splat(TreeView t, AccumView a, pg_filter_args f, int store_nee, uint64_t m,
                                                          const float *__restrict__ pos, const float *__restrict__ dir,
                                                          const float *__restrict__ radiance,
                                                          const float *__restrict__ wo_pdf,
                                                          const float *__restrict__ dir_nee,
                                                          const float *__restrict__ nee_lum,
                                                          const uint32_t *__restrict__ d_count)
{
	PG_FILTER_LDS();
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	const uint64_t n_valid = d_count ? (uint64_t)*d_count : m; // plane stride stays m
	const bool valid = i < n_valid && i < m;
	float x = 0.0f, y = 0.0f, z = 0.0f, dx = 0.0f, dy = 0.0f, rad = 0.0f, wp = 0.0f, nx = 0.0f, ny = 0.0f, nl = 0.0f;
	if (valid) {
		x = pos[i]; y = pos[m + i]; z = pos[2 * m + i];
		dx = dir[i]; dy = dir[m + i];
		rad = radiance[i]; wp = wo_pdf[i];
		if (store_nee) { nx = dir_nee[i]; ny = dir_nee[m + i]; nl = nee_lum[i]; }
	}
	splat_filtered<kOverlap>(t, a, s_planes, f, store_nee, valid, (uint32_t)i, x, y, z, dx, dy, rad, wp, nx, ny, nl, s_q, len, s_val, s_ptr);
	queue_drain(a, s_q, len, s_val, s_ptr);
}

// the dense record buffer (k_process_and_splat's loop over the tiles, pg_kernels_splat.hip); record number = dense slot g
template <bool kOverlap>
__global__ __launch_bounds__(kBlock) void k_filter_process_and_splat(TreeView t, AccumView a, pg_filter_args f, int store_nee,
                                                                      uint64_t num_rays, int32_t max_depth,
                                                                      const float *__restrict__ l_final, pg_dense_records r)
{
	PG_FILTER_LDS();
	const uint64_t S = num_rays * (uint64_t)max_depth;
	stage_kd_planes(s_planes, t);
	for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < S; base += (uint64_t)gridDim.x * kBlock) {
		const uint64_t g = base + threadIdx.x;
		float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
		bool keep = false;
		if (g < S) keep = process_slot(g, S, num_rays, g / (uint64_t)max_depth, r.active[g] != 0, l_final, r, radiance, nee_lum, wp);
		float x = 0.0f, y = 0.0f, z = 0.0f, dx = 0.0f, dy = 0.0f, nx = 0.0f, ny = 0.0f;
		if (keep) {
			x = r.position[g]; y = r.position[S + g]; z = r.position[2 * S + g];
			dx = r.direction[g]; dy = r.direction[S + g];
			nx = r.direction_nee[g]; ny = r.direction_nee[S + g];
		}
		splat_filtered<kOverlap>(t, a, s_planes, f, store_nee, keep, (uint32_t)g, x, y, z, dx, dy, radiance, wp, nx, ny, nee_lum, s_q, len, s_val,
		               s_ptr);
	}
	queue_drain(a, s_q, len, s_val, s_ptr);
}

// The renderer's own record list with its vertex geometry (pg_render_record_geometry) through the filters: every kept entry
// (process_list_entry; such a pass keeps a path's final radiance in l_final_q) is the record pg_process_and_splat would have
// found in dense slot ray * max_depth + depth of the reference's buffer, and that slot (modulo 2^32) is its record number
// for the jitter.
template <bool kOverlap>
__global__ __launch_bounds__(kBlock) void k_filter_splat_list(TreeView t, AccumView a, pg_filter_args f, int store_nee, uint64_t num_rays,
                                                              int32_t max_depth, const uint4 *__restrict__ l_final_q, pg_list_records r,
                                                              pg_list_geometry geo, const uint32_t *__restrict__ live_count)
{
	PG_FILTER_LDS();
	const uint64_t S = num_rays * (uint64_t)max_depth;
	const uint64_t total = list_entries(num_rays, max_depth, live_count);
	stage_kd_planes(s_planes, t);
	for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < total; base += (uint64_t)gridDim.x * kBlock) {
		const uint64_t g = base + threadIdx.x;
		float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
		uint32_t ray = 0;
		const bool keep = g < total && process_list_entry(g, S, num_rays, nullptr, l_final_q, r, ray, radiance, nee_lum, wp);
		float x = 0.0f, y = 0.0f, z = 0.0f, dx = 0.0f, dy = 0.0f, nx = 0.0f, ny = 0.0f;
		uint32_t index = 0;
		if (keep) {
			x = geo.position[g]; y = geo.position[S + g]; z = geo.position[2 * S + g];
			dx = geo.direction[g]; dy = geo.direction[S + g];
			nx = geo.direction_nee[g]; ny = geo.direction_nee[S + g];
			index = (uint32_t)((uint64_t)ray * (uint64_t)max_depth + geo.depth[g]);
		}
		splat_filtered<kOverlap>(t, a, s_planes, f, store_nee, keep, index, x, y, z, dx, dy, radiance, wp, nx, ny, nee_lum, s_q, len, s_val, s_ptr);
	}
	queue_drain(a, s_q, len, s_val, s_ptr);
}

#undef PG_FILTER_LDS

// the kernels of PG_SPATIAL_OVERLAP_BOX are instances of their own: those of the other filters carry nothing of its walk
static inline bool overlap(const pg_filter_args &f) { return f.spatial == PG_SPATIAL_OVERLAP_BOX; }

void launch_splat_list_filtered(const TreeView &t, const AccumView &a, const pg_filter_args &f, int store_nee, uint64_t num_rays,
                                int32_t max_depth, const uint4 *l_final_q, const pg_list_records &rec, const pg_list_geometry &geo,
                                const uint32_t *live_count, int n_cus, hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	if (S == 0) return;
	const auto kernel = overlap(f) ? k_filter_splat_list<true> : k_filter_splat_list<false>;
	hipLaunchKernelGGL(kernel, strided_grid(S, n_cus), dim3(kBlock), 0, s, t, a, f, store_nee, num_rays, max_depth, l_final_q, rec, geo,
	                   live_count);
}

void launch_splat_filtered(const TreeView &t, const AccumView &a, const pg_filter_args &f, int store_nee, uint64_t m,
                           const pg_records &rec, const uint32_t *d_count, hipStream_t s)
{
	if (m == 0) return;
	const auto kernel = overlap(f) ? k_filter_splat<true> : k_filter_splat<false>;
	hipLaunchKernelGGL(kernel, grid_for(m), dim3(kBlock), 0, s, t, a, f, store_nee, m, rec.position, rec.direction,
	                   rec.radiance, rec.wo_pdf, rec.direction_nee, rec.radiance_nee_lum, d_count);
}

void launch_process_and_splat_filtered(const TreeView &t, const AccumView &a, const pg_filter_args &f, int store_nee,
                                       uint64_t num_rays, int32_t max_depth, const float *l_final, const pg_dense_records &rec,
                                       int n_cus, hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	if (S == 0) return;
	const auto kernel = overlap(f) ? k_filter_process_and_splat<true> : k_filter_process_and_splat<false>;
	hipLaunchKernelGGL(kernel, strided_grid(S, n_cus), dim3(kBlock), 0, s, t, a, f, store_nee, num_rays, max_depth, l_final, rec);
}

} // namespace pg
