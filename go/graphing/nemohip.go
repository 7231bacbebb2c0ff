// Package graphing: the drop-in for the reference's graphing package
// (at15/nemo graphing/*.go).  This file replaces the Cypher-carrying files
// (helpers.go, pre-post-prov.go, preprocessing.go, prototype.go,
// differential-provenance.go, the two query functions of corrections.go,
// extensions.go); diagrams.go, hazard-analysis.go and corrections.go's string
// synthesis stay.  Every Neo4j round trip is a call into libnemohip's C ABI
// (include/nemohip.h).  See go/README.md for where the file goes and the one
// refactor of corrections.go it needs.
package graphing

/*
#cgo CFLAGS: -I${SRCDIR}/../third_party/nemohip/include
#cgo LDFLAGS: -L${SRCDIR}/../third_party/nemohip/nemo_amd -lnemohip -L/opt/rocm/lib -lamdhip64 -lrccl -Wl,-rpath,/opt/rocm/lib
#include <stdlib.h>
#include "nemohip.h"
*/
import "C"

import (
	"fmt"
	"sort"
	"strings"
	"unsafe"

	"github.com/awalterschulze/gographviz"
	"github.com/johnnadratowski/golang-neo4j-bolt-driver/structures/graph"

	fi "github.com/numbleroot/nemo/faultinjectors"
)

// Neo4J keeps its name and its exported field so main.go:95 (&gr.Neo4J{}) is
// untouched; it no longer talks to Neo4j (pre-post-prov.go:16-20).
type Neo4J struct {
	Runs []*fi.Run

	ctx     *C.nemo_ctx
	tables  []string          // interned table names, id = index
	tableID map[string]uint32
	labels  []string          // interned labels (exact interning, never a hash)
	labelID map[string]uint32
	runIdx  map[uint]int      // Run.Iteration -> run index (graph 2r = pre, 2r+1 = post)
	graphs  []*provGraph      // per graph g, node-index order
	chains  map[int][][2]uint32 // accepted @next chains per graph: (head, tail) by k
	red     *reduction          // last nemo_protos_finalize
}

// One loaded provenance graph: loadProv creates goals first, then rules
// (pre-post-prov.go:27-58,90-118), so local node i < len(Goals) is goal i.
type provGraph struct {
	iter     uint
	cond     string
	goals    []fi.Goal
	rules    []fi.Rule
	src, dst []uint32 // the loaded edges (local indices): the raw graph's relationships
}

func (p *provGraph) n() int { return len(p.goals) + len(p.rules) }

type reduction struct {
	achieved, nRuns uint32
	inter, union    []uint32
	preHolds        uint64
}

func (n *Neo4J) err(rc C.int) error {
	if rc == C.NEMO_OK {
		return nil
	}
	return fmt.Errorf("%s", C.GoString(C.nemo_last_error(n.ctx)))
}

func (n *Neo4J) intern(tab *[]string, ids map[string]uint32, s string) uint32 {
	if id, ok := ids[s]; ok {
		return id
	}
	id := uint32(len(*tab))
	*tab = append(*tab, s)
	ids[s] = id
	return id
}

func typeClass(t string) uint32 {
	switch t {
	case "next":
		return C.NEMO_TYPE_NEXT
	case "async":
		return C.NEMO_TYPE_ASYNC
	}
	return C.NEMO_TYPE_OTHER
}

// ---- helpers.go ---------------------------------------------------------------

// InitGraphDB (helpers.go:17-55): no docker-compose, no 10 s sleep, no Bolt;
// boltURI is accepted and ignored.  One node context over every GPU of the
// node: the corpus is run-sharded inside the library (include/nemohip.h).
func (n *Neo4J) InitGraphDB(boltURI string, runs []*fi.Run) error {
	if rc := C.nemo_ctx_create_node(0, nil, &n.ctx); rc != C.NEMO_OK {
		return fmt.Errorf("nemo_ctx_create_node: status %d", int(rc))
	}
	n.Runs = runs
	n.tableID, n.labelID = map[string]uint32{}, map[string]uint32{}
	n.runIdx = map[uint]int{}
	for r, run := range runs {
		n.runIdx[run.Iteration] = r
	}
	return nil
}

// CloseDB (helpers.go:58-86).
func (n *Neo4J) CloseDB() error {
	C.nemo_ctx_destroy(n.ctx)
	n.ctx = nil
	return nil
}

// ---- pre-post-prov.go -----------------------------------------------------------

// LoadRawProvenance (pre-post-prov.go:247-285): loadProv for every run's pre
// and post graph as interning into one nemo_corpus, one load (CSR build, the
// reference's validations, Kahn levels on the device), one markConditionHolds.
func (n *Neo4J) LoadRawProvenance() error {
	R := len(n.Runs)
	iters := make([]C.uint32_t, R)
	nodeOff, edgeOff := []C.uint64_t{0}, []C.uint64_t{0}
	var words, labels, ranks, src, dst []C.uint32_t
	n.graphs = n.graphs[:0]
	for r, run := range n.Runs {
		iters[r] = C.uint32_t(run.Iteration)
		for _, cond := range []string{"pre", "post"} {
			prov := run.PreProv
			if cond == "post" {
				prov = run.PostProv
			}
			if prov == nil {
				prov = &fi.ProvData{}
			}
			g := &provGraph{iter: run.Iteration, cond: cond, goals: prov.Goals, rules: prov.Rules}
			index := make(map[string]uint32, g.n())
			ids := make([]string, 0, g.n())
			for _, goal := range prov.Goals {
				index[goal.ID] = uint32(len(ids))
				ids = append(ids, goal.ID)
				words = append(words, C.uint32_t(n.intern(&n.tables, n.tableID, goal.Table)))
				labels = append(labels, C.uint32_t(n.intern(&n.labels, n.labelID, goal.Label)))
			}
			// Goal.id IS UNIQUE (pre-post-prov.go:66-81): a duplicate is not a second node
			nGoals := len(index)
			if nGoals != len(prov.Goals) {
				return fmt.Errorf("Run %d: inserted number of goals (%d) does not equal number of antecedent provenance goals (%d)", run.Iteration, nGoals, len(prov.Goals))
			}
			for _, rule := range prov.Rules {
				index[rule.ID] = uint32(len(ids))
				ids = append(ids, rule.ID)
				w := C.NEMO_NODE_RULE | typeClass(rule.Type)<<C.NEMO_TYPE_SHIFT | n.intern(&n.tables, n.tableID, rule.Table)
				words = append(words, C.uint32_t(w))
				labels = append(labels, C.uint32_t(n.intern(&n.labels, n.labelID, rule.Label)))
			}
			if len(index)-nGoals != len(prov.Rules) { // Rule.id IS UNIQUE (:126-141)
				return fmt.Errorf("Run %d: inserted number of rules (%d) does not equal number of antecedent provenance rules (%d)", run.Iteration, len(index)-nGoals, len(prov.Rules))
			}
			// rank of each ID inside the graph: the canonical @next tie-break (DESIGN.md §1)
			order := make([]int, len(ids))
			for i := range order {
				order[i] = i
			}
			sort.Slice(order, func(a, b int) bool { return ids[order[a]] < ids[order[b]] })
			rank := make([]C.uint32_t, len(ids))
			for pos, i := range order {
				rank[i] = C.uint32_t(pos)
			}
			ranks = append(ranks, rank...)
			// edges: direction by strings.Contains(From, "goal") (:173); a missing
			// endpoint or a duplicate creates no relationship, and the count check
			// of :208-210 then fails exactly as the reference's does
			seen := map[[2]uint32]bool{}
			created := 0
			for _, e := range prov.Edges {
				u, okU := index[e.From]
				v, okV := index[e.To]
				fromGoal := strings.Contains(e.From, "goal")
				if !okU || !okV || (int(u) < len(prov.Goals)) != fromGoal || (int(v) < len(prov.Goals)) == fromGoal ||
					seen[[2]uint32{u, v}] {
					continue
				}
				seen[[2]uint32{u, v}] = true
				src = append(src, C.uint32_t(u))
				dst = append(dst, C.uint32_t(v))
				g.src = append(g.src, u)
				g.dst = append(g.dst, v)
				created++
			}
			if created != len(prov.Edges) {
				return fmt.Errorf("Run %d: inserted number of edges (%d) does not equal number of antecedent provenance edges (%d)",
					run.Iteration, created, len(prov.Edges))
			}
			nodeOff = append(nodeOff, C.uint64_t(len(words)))
			edgeOff = append(edgeOff, C.uint64_t(len(src)))
			n.graphs = append(n.graphs, g)
		}
	}
	n.intern(&n.tables, n.tableID, "pre")
	n.intern(&n.tables, n.tableID, "post")
	var corpus C.nemo_corpus
	corpus.n_runs = C.uint32_t(R)
	corpus.n_tables = C.uint32_t(len(n.tables))
	corpus.table_pre = C.uint32_t(n.tableID["pre"])
	corpus.table_post = C.uint32_t(n.tableID["post"])
	corpus.iteration = cArray(iters)
	corpus.node_off, corpus.edge_off = cArray(nodeOff), cArray(edgeOff)
	corpus.node_word, corpus.label, corpus.id_rank = cArray(words), cArray(labels), cArray(ranks)
	corpus.edge_src, corpus.edge_dst = cArray(src), cArray(dst)
	defer freeCorpus(&corpus)
	if err := n.err(C.nemo_load_corpus(n.ctx, &corpus)); err != nil {
		return err
	}
	return n.err(C.nemo_mark_holds(n.ctx))
}

// cArray copies a Go slice to C memory (cgo forbids Go pointers to Go pointers).
func cArray[T any](s []T) *T {
	if len(s) == 0 {
		return nil
	}
	var z T
	p := (*T)(C.malloc(C.size_t(len(s)) * C.size_t(unsafe.Sizeof(z))))
	copy(unsafe.Slice(p, len(s)), s)
	return p
}

func freeCorpus(c *C.nemo_corpus) {
	for _, p := range []unsafe.Pointer{unsafe.Pointer(c.iteration), unsafe.Pointer(c.node_off),
		unsafe.Pointer(c.edge_off), unsafe.Pointer(c.node_word), unsafe.Pointer(c.label),
		unsafe.Pointer(c.id_rank), unsafe.Pointer(c.edge_src), unsafe.Pointer(c.edge_dst)} {
		C.free(p)
	}
}

// ---- preprocessing.go -------------------------------------------------------------

// SimplifyProv (preprocessing.go:351-387): cleanCopyProv + collapseNextChains
// of every loaded run on the device; the accepted chains come back once.
func (n *Neo4J) SimplifyProv(iters []uint) error {
	for _, it := range iters {
		if _, ok := n.runIdx[it]; !ok {
			return fmt.Errorf("SimplifyProv: run %d was not loaded", it)
		}
	}
	if err := n.err(C.nemo_simplify(n.ctx)); err != nil {
		return err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_chains(n.ctx, nil, 0, &cnt)); err != nil {
		return err
	}
	ch := make([]C.nemo_chain, int(cnt)+1)
	if err := n.err(C.nemo_fetch_chains(n.ctx, &ch[0], cnt, &cnt)); err != nil {
		return err
	}
	n.chains = map[int][][2]uint32{}
	for _, c := range ch[:cnt] { // ordered by (graph, k)
		g := int(c.graph)
		n.chains[g] = append(n.chains[g], [2]uint32{uint32(c.head), uint32(c.tail)})
	}
	return nil
}

// ---- node properties (what loadProv stored, plus the device flags) ---------------

func rewriteRun(id string, old, new uint) string { // the `id`:"run_<old> rewrite (preprocessing.go:33-45)
	pfx := fmt.Sprintf("run_%d", old)
	if strings.HasPrefix(id, pfx) {
		return fmt.Sprintf("run_%d", new) + id[len(pfx):]
	}
	return id
}

// node returns the bolt-driver graph.Node createDOT reads (diagrams.go:41-83):
// labels "Goal"/"Rule", properties id, label, table, type, condition_holds,
// time.  run != nil re-prefixes the ID like the clean (1000+i) and diff
// (2000+f) copies.  Local index V_g+k is collapsed rule k (preprocessing.go:249-252).
func (n *Neo4J) node(g int, i uint32, flags []uint8, run *uint) graph.Node {
	pg := n.graphs[g]
	V := uint32(pg.n())
	if i >= V {
		k := i - V
		head := n.chains[g][k][0]
		table := pg.rules[int(head)-len(pg.goals)].Table
		lab := table + "_collapsed"
		return graph.Node{Labels: []string{"Rule"}, Properties: map[string]interface{}{
			"id": fmt.Sprintf("run_%d_%s_%s_%d", 1000+pg.iter, pg.cond, lab, k), "label": lab,
			"table": table, "type": "collapsed"}}
	}
	if int(i) < len(pg.goals) {
		goal := pg.goals[i]
		id := goal.ID
		if run != nil {
			id = rewriteRun(id, pg.iter, *run)
		}
		return graph.Node{Labels: []string{"Goal"}, Properties: map[string]interface{}{
			"id": id, "label": goal.Label, "table": goal.Table, "time": goal.Time,
			"condition_holds": flags[i]&C.NEMO_F_HOLDS != 0}}
	}
	rule := pg.rules[int(i)-len(pg.goals)]
	id := rule.ID
	if run != nil {
		id = rewriteRun(id, pg.iter, *run)
	}
	return graph.Node{Labels: []string{"Rule"}, Properties: map[string]interface{}{
		"id": id, "label": rule.Label, "table": rule.Table, "type": rule.Type}}
}

func (n *Neo4J) flags(g int) ([]uint8, error) {
	f := make([]uint8, n.graphs[g].n()+1)
	if err := n.err(C.nemo_fetch_node_flags(n.ctx, C.uint32_t(g), C.uint32_t(g+1), (*C.uint8_t)(&f[0]), C.uint64_t(len(f)))); err != nil {
		return nil, err
	}
	return f, nil
}

// paths turns pulled slot `slot` of graph g into the []graph.Path rows
// createDOT / createDiffDot consume, in (source, target) order.
func (n *Neo4J) paths(slot uint32, g int, run *uint) ([]graph.Path, error) {
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_pulled(n.ctx, C.uint32_t(slot), nil, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	s, d := make([]uint32, cnt+1), make([]uint32, cnt+1)
	if err := n.err(C.nemo_fetch_pulled(n.ctx, C.uint32_t(slot), (*C.uint32_t)(&s[0]), (*C.uint32_t)(&d[0]), cnt, &cnt)); err != nil {
		return nil, err
	}
	return n.edgeRows(s[:cnt], d[:cnt], g, run)
}

// rawPaths: the rows of raw graph g (run i, pre-post-prov.go:298-301) are its
// loaded edges, which the binding holds, so no device pull is needed.
func (n *Neo4J) rawPaths(g int) ([]graph.Path, error) {
	return n.edgeRows(n.graphs[g].src, n.graphs[g].dst, g, nil)
}

func (n *Neo4J) edgeRows(s, d []uint32, g int, run *uint) ([]graph.Path, error) {
	cnt := len(s)
	idx := make([]int, cnt)
	for i := range idx {
		idx[i] = i
	}
	sort.Slice(idx, func(a, b int) bool {
		if s[idx[a]] != s[idx[b]] {
			return s[idx[a]] < s[idx[b]]
		}
		return d[idx[a]] < d[idx[b]]
	})
	fl, err := n.flags(g)
	if err != nil {
		return nil, err
	}
	out := make([]graph.Path, 0, cnt)
	for _, j := range idx {
		out = append(out, graph.Path{Nodes: []graph.Node{n.node(g, s[j], fl, run), n.node(g, d[j], fl, run)},
			Relationships: []graph.UnboundRelationship{{Type: "DUETO"}}})
	}
	return out, nil
}

// PullPrePostProv (pre-post-prov.go:288-459): raw graphs (run i) and
// simplified graphs (run 1000+i) of every run, through createDOT (unchanged).
func (n *Neo4J) PullPrePostProv() ([]*gographviz.Graph, []*gographviz.Graph, []*gographviz.Graph, []*gographviz.Graph, error) {
	R := len(n.Runs)
	pre, post := make([]*gographviz.Graph, R), make([]*gographviz.Graph, R)
	preC, postC := make([]*gographviz.Graph, R), make([]*gographviz.Graph, R)
	var err error
	var rows []graph.Path
	for r := 0; r < R; r++ {
		if rows, err = n.rawPaths(2 * r); err != nil {
			return nil, nil, nil, nil, err
		}
		if pre[r], err = createDOT(rows, "pre"); err != nil {
			return nil, nil, nil, nil, err
		}
		if rows, err = n.rawPaths(2*r + 1); err != nil {
			return nil, nil, nil, nil, err
		}
		if post[r], err = createDOT(rows, "post"); err != nil {
			return nil, nil, nil, nil, err
		}
	}
	if err = n.err(C.nemo_pull_edges(n.ctx, 1)); err != nil {
		return nil, nil, nil, nil, err
	}
	for r := 0; r < R; r++ {
		clean := 1000 + n.Runs[r].Iteration
		if rows, err = n.paths(uint32(2*r), 2*r, &clean); err != nil {
			return nil, nil, nil, nil, err
		}
		if preC[r], err = createDOT(rows, "pre"); err != nil {
			return nil, nil, nil, nil, err
		}
		if rows, err = n.paths(uint32(2*r+1), 2*r+1, &clean); err != nil {
			return nil, nil, nil, nil, err
		}
		if postC[r], err = createDOT(rows, "post"); err != nil {
			return nil, nil, nil, nil, err
		}
	}
	return pre, post, preC, postC, nil
}

// ---- prototype.go -------------------------------------------------------------------

func (n *Neo4J) reduce(success []uint) (*reduction, error) {
	s := make([]C.uint32_t, len(success)+1)
	for i, it := range success {
		s[i] = C.uint32_t(it)
	}
	if err := n.err(C.nemo_protos_partial(n.ctx, &s[0], C.size_t(len(success)), nil)); err != nil {
		return nil, err
	}
	T := len(n.tables)
	inter, uni := make([]C.uint32_t, T+1), make([]C.uint32_t, T+1)
	var achvd, ni, nu, nr C.uint32_t
	var ph C.uint64_t
	if err := n.err(C.nemo_protos_finalize(n.ctx, nil, &achvd, &inter[0], &ni, &uni[0], &nu, &ph, &nr)); err != nil {
		return nil, err
	}
	red := &reduction{achieved: uint32(achvd), nRuns: uint32(nr), preHolds: uint64(ph)}
	for _, t := range inter[:ni] {
		red.inter = append(red.inter, uint32(t))
	}
	for _, t := range uni[:nu] {
		red.union = append(red.union, uint32(t))
	}
	n.red = red
	return red, nil
}

func (n *Neo4J) tableNames(ids []uint32) []string {
	out := make([]string, len(ids))
	for i, t := range ids {
		out[i] = n.tables[t]
	}
	return out
}

func codeWrap(ts []string) []string { // prototype.go:245-251
	out := make([]string, len(ts))
	for i, t := range ts {
		out[i] = fmt.Sprintf("<code>%s</code>", t)
	}
	return out
}

// missingFrom (prototype.go:141-206): proto entries absent from the failed
// run's simplified post graph, in proto order, wrapped in <code> (:196).
func (n *Neo4J) missingFrom(proto []uint32, failedIter uint) ([]string, error) {
	p := make([]C.uint32_t, len(proto)+1)
	for i, t := range proto {
		p[i] = C.uint32_t(t)
	}
	out := make([]C.uint32_t, len(proto)+1)
	var cnt C.uint32_t
	if err := n.err(C.nemo_missing_from(n.ctx, C.uint32_t(failedIter), &p[0], C.uint32_t(len(proto)), &out[0], &cnt)); err != nil {
		return nil, err
	}
	ids := make([]uint32, cnt)
	for i := range ids {
		ids[i] = uint32(out[i])
	}
	return codeWrap(n.tableNames(ids)), nil
}

// CreatePrototypes (prototype.go:209-256): extractProtos on the device,
// inter/union from the (all-reduced) vector, missingFrom per failed run,
// <code> wrapping after the missing computation (:245-251).
func (n *Neo4J) CreatePrototypes(iters []uint, failedIters []uint) ([]string, [][]string, []string, [][]string, error) {
	if len(iters) == 0 { // the reference indexes iterProv[0] (prototype.go:80) and panics
		return nil, nil, nil, nil, fmt.Errorf("no successful runs")
	}
	red, err := n.reduce(iters)
	if err != nil {
		return nil, nil, nil, nil, err
	}
	interMiss, unionMiss := make([][]string, len(failedIters)), make([][]string, len(failedIters))
	for i, f := range failedIters {
		if interMiss[i], err = n.missingFrom(red.inter, f); err != nil {
			return nil, nil, nil, nil, err
		}
		if unionMiss[i], err = n.missingFrom(red.union, f); err != nil {
			return nil, nil, nil, nil, err
		}
	}
	return codeWrap(n.tableNames(red.inter)), interMiss, codeWrap(n.tableNames(red.union)), unionMiss, nil
}

// ---- differential-provenance.go -------------------------------------------------------

// CreateNaiveDiffProv (differential-provenance.go:18-243): nemo_diffprov in
// NEMO_DIFF_REFERENCE (the in-place ###RUN### substitution of :43; the node
// context broadcasts failedRuns[0]'s label set to every device), the D masks,
// the missing rules (Missing.Goals = all D-children of each, the `leaf`
// rebinding of :93-95), the D edges (Q24) and the failed run's edges, then
// createDiffDot (unchanged).  `symmetric` is unused, as in the reference.
func (n *Neo4J) CreateNaiveDiffProv(symmetric bool, failedRuns []uint, successPostProv *gographviz.Graph) ([]*gographviz.Graph, []*gographviz.Graph, [][]*fi.Missing, error) {
	f := make([]C.uint32_t, len(failedRuns)+1)
	for i, it := range failedRuns {
		f[i] = C.uint32_t(it)
	}
	if err := n.err(C.nemo_diffprov(n.ctx, &f[0], C.size_t(len(failedRuns)), C.NEMO_DIFF_REFERENCE)); err != nil {
		return nil, nil, nil, err
	}
	g0 := 2*n.runIdx[0] + 1
	V0 := n.graphs[g0].n()
	var masks *C.uint8_t
	var ne, v0 C.uint64_t
	if err := n.err(C.nemo_diff_masks_view(n.ctx, &masks, &ne, &v0)); err != nil {
		return nil, nil, nil, err
	}
	maskOf := func(e int) []uint8 {
		return unsafe.Slice((*uint8)(unsafe.Pointer(masks)), int(ne)*V0)[e*V0 : (e+1)*V0]
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_missing(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, nil, nil, err
	}
	rows := make([]C.nemo_missing, cnt+1)
	if err := n.err(C.nemo_fetch_missing(n.ctx, &rows[0], cnt, &cnt)); err != nil {
		return nil, nil, nil, err
	}
	// D-children of every missing rule from run 0's post edges (the interned arrays)
	children := n.childrenOf(g0)
	fl, err := n.flags(g0)
	if err != nil {
		return nil, nil, nil, err
	}
	missing := make([][]*fi.Missing, len(failedRuns))
	for _, row := range rows[:cnt] {
		e, rule := int(row.entry), uint32(row.rule)
		run := 2000 + failedRuns[e]
		rn := n.node(g0, rule, fl, &run)
		m := &fi.Missing{Rule: ruleOf(rn)}
		for _, ch := range children[rule] {
			if maskOf(e)[ch] != 0 {
				gn := n.node(g0, ch, fl, &run)
				m.Goals = append(m.Goals, goalOf(gn))
			}
		}
		missing[e] = append(missing[e], m)
	}
	if err := n.err(C.nemo_pull_edges(n.ctx, 2)); err != nil {
		return nil, nil, nil, err
	}
	diffEdges := make([][]graph.Path, len(failedRuns))
	for e, it := range failedRuns {
		run := 2000 + it
		if diffEdges[e], err = n.paths(uint32(e), g0, &run); err != nil {
			return nil, nil, nil, err
		}
	}
	diffDots, failedDots := make([]*gographviz.Graph, len(failedRuns)), make([]*gographviz.Graph, len(failedRuns))
	for e, it := range failedRuns {
		gf := 2*n.runIdx[it] + 1
		failedRows, err := n.rawPaths(gf)
		if err != nil {
			return nil, nil, nil, err
		}
		diffDots[e], failedDots[e], err = createDiffDot(2000+it, diffEdges[e], it, failedRows, 0,
			successPostProv, missing[e])
		if err != nil {
			return nil, nil, nil, err
		}
	}
	return diffDots, failedDots, missing, nil
}

// PairDiff is the differential provenance of one pair of runs: what the base
// run's consequent provenance has that the other run lacks.
type PairDiff struct {
	Base, Other uint          // iterations
	Mask        []uint8       // one byte per node of the base run's post graph: 1 = in the diff
	Edges       []graph.Path  // the base run's post graph induced on Mask, in (source, target) order
	Surplus     []*fi.Missing // the surplus events: rules at the frontier of the diff, with their goals in it
}

// PairDiffProv compares arbitrary pairs of loaded runs (nemo_diffprov_pairs):
// pairs[e] = {base iteration, other iteration}.  The reference has no
// counterpart, it compares with run 0 only (differential-provenance.go:22-28,
// 82-98 are the two queries evaluated here between the pair).  The call is
// followed by the three fetches of the symmetric diff (INTEGRATION.md §8, §10).
func (n *Neo4J) PairDiffProv(pairs [][2]uint) ([]*PairDiff, error) {
	base, other := make([]C.uint32_t, len(pairs)+1), make([]C.uint32_t, len(pairs)+1)
	for e, p := range pairs {
		base[e], other[e] = C.uint32_t(p[0]), C.uint32_t(p[1])
	}
	if err := n.err(C.nemo_diffprov_pairs(n.ctx, &base[0], &other[0], C.size_t(len(pairs)))); err != nil {
		return nil, err
	}
	// ragged masks: entry e's bytes are out[off[e]:off[e+1]], over the base run's post graph
	off := make([]C.uint64_t, len(pairs)+1)
	var used C.uint64_t
	if err := n.err(C.nemo_fetch_sdiff_masks(n.ctx, &off[0], nil, 0, &used)); err != nil {
		return nil, err
	}
	out := make([]uint8, used+1)
	if err := n.err(C.nemo_fetch_sdiff_masks(n.ctx, nil, (*C.uint8_t)(&out[0]), used, &used)); err != nil {
		return nil, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_surplus(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	rows := make([]C.nemo_missing, cnt+1)
	if err := n.err(C.nemo_fetch_surplus(n.ctx, &rows[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	if err := n.err(C.nemo_pull_edges(n.ctx, 3)); err != nil {
		return nil, err
	}
	res := make([]*PairDiff, len(pairs))
	for e, p := range pairs {
		gb := 2*n.runIdx[p[0]] + 1
		d := &PairDiff{Base: p[0], Other: p[1], Mask: out[off[e]:off[e+1]]}
		var err error
		if d.Edges, err = n.paths(uint32(e), gb, nil); err != nil {
			return nil, err
		}
		res[e] = d
	}
	// `rule` is local to the entry's base run's post graph; an event's goals are the rule's children in the mask
	children, flagsOf := map[int]map[uint32][]uint32{}, map[int][]uint8{}
	for _, row := range rows[:cnt] {
		e, rule := int(row.entry), uint32(row.rule)
		gb := 2*n.runIdx[pairs[e][0]] + 1
		if _, ok := children[gb]; !ok {
			children[gb] = n.childrenOf(gb)
			fl, err := n.flags(gb)
			if err != nil {
				return nil, err
			}
			flagsOf[gb] = fl
		}
		m := &fi.Missing{Rule: ruleOf(n.node(gb, rule, flagsOf[gb], nil))}
		for _, ch := range children[gb][rule] {
			if res[e].Mask[ch] != 0 {
				m.Goals = append(m.Goals, goalOf(n.node(gb, ch, flagsOf[gb], nil)))
			}
		}
		res[e].Surplus = append(res[e].Surplus, m)
	}
	return res, nil
}

// NearestRun names, for one query run, the candidate run whose derived post
// goals are nearest to its own.
type NearestRun struct {
	Query       uint // iteration
	Nearest     uint // iteration of the nearest candidate (valid only if Found)
	Found       bool // false: no candidate but the query itself
	Dist        uint // labels of post goals only one of the two runs derived
	OnlyQuery   uint // ... that only the query derived
	OnlyNearest uint // ... that only the candidate derived
}

// NearestRuns picks the partner of every query run for PairDiffProv
// (nemo_nearest_runs): the candidate whose set of post-goal labels differs
// least from the query's, ties to the earlier candidate, the query itself
// skipped.  The reference has no counterpart, it compares with run 0 only.
func (n *Neo4J) NearestRuns(queries, candidates []uint) ([]*NearestRun, error) {
	qs, cs := make([]C.uint32_t, len(queries)+1), make([]C.uint32_t, len(candidates)+1)
	for i, it := range queries {
		qs[i] = C.uint32_t(it)
	}
	for j, it := range candidates {
		cs[j] = C.uint32_t(it)
	}
	if err := n.err(C.nemo_nearest_runs(n.ctx, &qs[0], C.size_t(len(queries)), &cs[0], C.size_t(len(candidates)))); err != nil {
		return nil, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_nearest(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	near := make([]C.nemo_nearest, cnt+1)
	if err := n.err(C.nemo_fetch_nearest(n.ctx, &near[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	res := make([]*NearestRun, len(queries))
	for i, it := range queries {
		res[i] = &NearestRun{Query: it}
		if j := uint32(near[i].cand); j != ^uint32(0) {
			res[i].Nearest, res[i].Found = candidates[j], true
			res[i].Dist, res[i].OnlyQuery, res[i].OnlyNearest = uint(near[i].dist), uint(near[i].only_query), uint(near[i].only_cand)
		}
	}
	return res, nil
}

// KnockOut is one hypothesis of a knock-out analysis: a set of nodes of one
// provenance graph removed by assumption, and what that does to the graph read
// as an AND/OR circuit (a goal holds if any of its rule firings holds, a rule
// firing if all of its premises hold).
type KnockOut struct {
	Iteration uint   // the run
	Cond      string // "pre" or "post"
	Node      string // leaves mode: the ID of the sink goal knocked out; sets mode: ""
	Label     string // ... and its label
	Dead      uint   // dead nodes, the removed ones included
	RootsDead uint   // dead nodes of in-degree 0
	Roots     uint   // nodes of in-degree 0
	Lost      bool   // every root is dead: the outcome has no derivation left
}

func condIndex(cond string) C.int {
	if cond == "post" {
		return 1
	}
	return 0
}

// knockRows fetches the rows of the last knock-out call.
func (n *Neo4J) knockRows() ([]C.nemo_knock, error) {
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_knockout(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	rows := make([]C.nemo_knock, cnt+1)
	if err := n.err(C.nemo_fetch_knockout(n.ctx, &rows[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	return rows[:cnt], nil
}

func (n *Neo4J) knockOut(k C.nemo_knock) *KnockOut {
	p := n.graphs[int(k.graph)]
	res := &KnockOut{Iteration: p.iter, Cond: p.cond, Dead: uint(k.n_dead), RootsDead: uint(k.roots_dead), Roots: uint(k.n_roots)}
	res.Lost = k.n_roots > 0 && k.roots_dead == k.n_roots
	if v := int(k.node); uint32(k.node) != ^uint32(0) && v < len(p.goals) {
		res.Node, res.Label = p.goals[v].ID, p.goals[v].Label
	}
	return res
}

// KnockOutLeaves knocks out every sink goal (base fact) of the given runs'
// pre or post provenance, one at a time (nemo_knockout_leaves), and returns
// one record per sink goal, runs in list order.  It replaces the Cypher path
// query "is there still a derivation of post if this event is lost?"; the
// reference's graphing package has no counterpart.  The second result gives,
// per listed run, the first record and the number of records of that run
// (nemo_fetch_knockout_ranges).
func (n *Neo4J) KnockOutLeaves(iters []uint, cond string) ([]*KnockOut, [][2]uint64, error) {
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	if err := n.err(C.nemo_knockout_leaves(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), 0)); err != nil {
		return nil, nil, err
	}
	rows, err := n.knockRows()
	if err != nil {
		return nil, nil, err
	}
	first, count := make([]C.uint64_t, len(iters)+1), make([]C.uint32_t, len(iters)+1)
	if err := n.err(C.nemo_fetch_knockout_ranges(n.ctx, &first[0], &count[0], C.uint64_t(len(iters)))); err != nil {
		return nil, nil, err
	}
	res := make([]*KnockOut, len(rows))
	for h, k := range rows {
		res[h] = n.knockOut(k)
	}
	ranges := make([][2]uint64, len(iters))
	for i := range iters {
		ranges[i] = [2]uint64{uint64(first[i]), uint64(count[i])}
	}
	return res, ranges, nil
}

// KnockOutSets evaluates explicit hypotheses on one run's pre or post
// provenance (nemo_knockout_sets): sets[s] holds the local node indices
// (goals first, then rules, in loading order) removed under hypothesis s.
// With masks, the third result holds per hypothesis one byte per node,
// 1 = dead (nemo_fetch_knockout_mask).
func (n *Neo4J) KnockOutSets(iter uint, cond string, sets [][]uint32, masks bool) ([]*KnockOut, [][]byte, error) {
	off := make([]C.uint64_t, len(sets)+1)
	var nodes []C.uint32_t
	for s, set := range sets {
		for _, v := range set {
			nodes = append(nodes, C.uint32_t(v))
		}
		off[s+1] = C.uint64_t(len(nodes))
	}
	nodes = append(nodes, 0) // never empty: &nodes[0] below
	var flags C.uint32_t
	if masks {
		flags = C.NEMO_KO_MASKS
	}
	if err := n.err(C.nemo_knockout_sets(n.ctx, C.uint32_t(iter), condIndex(cond), &off[0], &nodes[0], C.size_t(len(sets)), flags)); err != nil {
		return nil, nil, err
	}
	rows, err := n.knockRows()
	if err != nil {
		return nil, nil, err
	}
	res := make([]*KnockOut, len(rows))
	var dead [][]byte
	for h, k := range rows {
		res[h] = n.knockOut(k)
		if masks {
			m := make([]byte, n.graphs[int(k.graph)].n()+1)
			if err := n.err(C.nemo_fetch_knockout_mask(n.ctx, C.uint64_t(h), (*C.uint8_t)(unsafe.Pointer(&m[0])), C.uint64_t(len(m)))); err != nil {
				return nil, nil, err
			}
			dead = append(dead, m[:len(m)-1])
		}
	}
	return res, dead, nil
}

// MinCut is one minimal cut of a run's provenance: a smallest set of nodes
// whose joint loss leaves no root of the graph with a derivation, while the
// loss of any proper subset does not.
type MinCut struct {
	Nodes  []uint32 // local node indices, in candidate-list order
	IDs    []string // their node IDs ("" for a rule)
	Labels []string // ... and labels
}

// MinCuts returns all minimal cuts of at most maxSize (1..3) nodes of one
// run's pre or post provenance among the candidates (nemo_min_cuts): local
// node indices of any kind, or nil for every sink goal (base fact) of the
// graph.  It answers "this run survives the loss of any one message; which
// pairs or triples of losses break it?", the question lineage-driven fault
// injection searches; the reference's graphing package has no counterpart.
// The cuts come sorted by size, then by the colex rank of their positions in
// the list of candidates that are no cut alone.  The second result holds, per
// size 1..3, the live candidates entering the round, the hypotheses evaluated
// and the minimal cuts found (nemo_fetch_min_cut_stats).
func (n *Neo4J) MinCuts(iter uint, cond string, candidates []uint32, maxSize uint) ([]*MinCut, [9]uint64, error) {
	var stats [9]uint64
	var list *C.uint32_t
	if candidates != nil {
		nodes := make([]C.uint32_t, len(candidates)+1) // never empty: &nodes[0] below
		for i, v := range candidates {
			nodes[i] = C.uint32_t(v)
		}
		list = &nodes[0]
	}
	if err := n.err(C.nemo_min_cuts(n.ctx, C.uint32_t(iter), condIndex(cond), list, C.size_t(len(candidates)), C.uint32_t(maxSize), 0)); err != nil {
		return nil, stats, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_min_cuts(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, stats, err
	}
	cuts := make([]C.nemo_cut, cnt+1)
	if err := n.err(C.nemo_fetch_min_cuts(n.ctx, &cuts[0], cnt, &cnt)); err != nil {
		return nil, stats, err
	}
	if err := n.err(C.nemo_fetch_min_cut_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, stats, err
	}
	p := n.graphs[2*n.runIdx[iter]+int(condIndex(cond))]
	res := make([]*MinCut, cnt)
	for k, cut := range cuts[:cnt] {
		m := &MinCut{}
		for j := 0; j < int(cut.size); j++ {
			v := uint32(cut.node[j])
			id, label := "", ""
			if int(v) < len(p.goals) {
				id, label = p.goals[v].ID, p.goals[v].Label
			}
			m.Nodes, m.IDs, m.Labels = append(m.Nodes, v), append(m.IDs, id), append(m.Labels, label)
		}
		res[k] = m
	}
	return res, stats, nil
}

// LineageCuts returns all minimal cuts of at most maxSize (1..8) nodes of one
// run's pre or post provenance among the candidates (nemo_lineage_cuts), as
// MinCuts does up to size 3, by the search lineage-driven fault injection
// makes: a fault set that does not defeat the outcome is extended only by the
// candidates that lie in the derivation it leaves.  The cuts come sorted by
// size, then by the colex order of their positions in the candidate list.  The
// second result holds, per size 0..8, the sets evaluated and the minimal cuts
// found (nemo_fetch_lineage_cut_stats).
func (n *Neo4J) LineageCuts(iter uint, cond string, candidates []uint32, maxSize uint) ([]*MinCut, [18]uint64, error) {
	var stats [18]uint64
	var list *C.uint32_t
	if candidates != nil {
		nodes := make([]C.uint32_t, len(candidates)+1) // never empty: &nodes[0] below
		for i, v := range candidates {
			nodes[i] = C.uint32_t(v)
		}
		list = &nodes[0]
	}
	if err := n.err(C.nemo_lineage_cuts(n.ctx, C.uint32_t(iter), condIndex(cond), list, C.size_t(len(candidates)), C.uint32_t(maxSize), 0)); err != nil {
		return nil, stats, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_lineage_cuts(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, stats, err
	}
	cuts := make([]C.nemo_lineage_cut, cnt+1)
	if err := n.err(C.nemo_fetch_lineage_cuts(n.ctx, &cuts[0], cnt, &cnt)); err != nil {
		return nil, stats, err
	}
	if err := n.err(C.nemo_fetch_lineage_cut_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, stats, err
	}
	p := n.graphs[2*n.runIdx[iter]+int(condIndex(cond))]
	res := make([]*MinCut, cnt)
	for k, cut := range cuts[:cnt] {
		m := &MinCut{}
		for j := 0; j < int(cut.size); j++ {
			v := uint32(cut.node[j])
			id, label := "", ""
			if int(v) < len(p.goals) {
				id, label = p.goals[v].ID, p.goals[v].Label
			}
			m.Nodes, m.IDs, m.Labels = append(m.Nodes, v), append(m.IDs, id), append(m.Labels, label)
		}
		res[k] = m
	}
	return res, stats, nil
}

// LabelKnockOut is the result of KnockoutLabels: one bit per (listed run, set).
type LabelKnockOut struct {
	Chunks int        // words per listed run: ceil(sets / 64)
	Lost   [][]uint64 // [run][chunk]: bit s%64 of word s/64 = the run's outcome is lost under set s
	Hit    [][]uint64 // ... = set s names a label some node of the run's graph carries
	NLost  []uint32   // per set: the listed runs it breaks (a run listed twice counts twice)
	NHit   []uint32   // per set: the listed runs it touches
}

// KnockoutLabels tests fault sets against every listed run's pre or post
// provenance in one call (nemo_knockout_labels).  A set names interned labels:
// "the message clock(a, b, 3, 4) is lost" is the same event in every run, so
// the same set stands for it on every graph.  A set removes every node whose
// label it names (sinksOnly: every base fact); the run's outcome is lost if no
// root of its graph keeps a derivation.  It answers "in which other good runs
// are run 0's cuts cuts too?" and "which single event breaks the most runs?"
// without translating labels to node indices per run; the reference's graphing
// package has no counterpart.
func (n *Neo4J) KnockoutLabels(iters []uint, cond string, sets [][]uint32, sinksOnly bool) (*LabelKnockOut, error) {
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	off := make([]C.uint64_t, len(sets)+1)
	var labels []C.uint32_t
	for s, set := range sets {
		for _, l := range set {
			labels = append(labels, C.uint32_t(l))
		}
		off[s+1] = C.uint64_t(len(labels))
	}
	labels = append(labels, 0) // never empty: &labels[0] below
	var flags C.uint32_t
	if sinksOnly {
		flags = C.NEMO_KL_SINKS
	}
	if err := n.err(C.nemo_knockout_labels(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), &off[0], &labels[0], C.size_t(len(sets)), flags)); err != nil {
		return nil, err
	}
	res := &LabelKnockOut{Chunks: (len(sets) + 63) / 64}
	words := len(iters) * res.Chunks
	lost, hit := make([]C.uint64_t, words+1), make([]C.uint64_t, words+1)
	if err := n.err(C.nemo_fetch_knockout_labels(n.ctx, &lost[0], &hit[0], C.uint64_t(words))); err != nil {
		return nil, err
	}
	nLost, nHit := make([]C.uint32_t, len(sets)+1), make([]C.uint32_t, len(sets)+1)
	if err := n.err(C.nemo_fetch_knockout_label_counts(n.ctx, &nLost[0], &nHit[0], C.uint64_t(len(sets)))); err != nil {
		return nil, err
	}
	for i := range iters {
		l, h := make([]uint64, res.Chunks), make([]uint64, res.Chunks)
		for c := 0; c < res.Chunks; c++ {
			l[c], h[c] = uint64(lost[i*res.Chunks+c]), uint64(hit[i*res.Chunks+c])
		}
		res.Lost, res.Hit = append(res.Lost, l), append(res.Hit, h)
	}
	for s := range sets {
		res.NLost, res.NHit = append(res.NLost, uint32(nLost[s])), append(res.NHit, uint32(nHit[s]))
	}
	return res, nil
}

// LabelCut is one minimal cut by label: a smallest set of events whose joint
// loss defeats the outcome on at least the asked number of listed runs.
type LabelCut struct {
	Labels []uint32 // interned labels, in candidate-list order
	NLost  uint32   // the listed runs it breaks (a run listed twice counts twice)
}

// MinLabelCuts searches where KnockoutLabels evaluates (nemo_min_label_cuts):
// among the candidate labels it returns every minimal set of at most maxSize
// (1..3) events whose loss defeats the outcome on at least minRuns of the
// listed runs' pre or post provenance (0: on every one of them).  It is the
// question of lineage-driven fault injection across runs; the reference's
// graphing package has no counterpart.  The cuts come sorted by size, then by
// the colex rank of their positions in the list of live candidates.  The
// second result holds, per size 1..3, the live candidates entering the round,
// the hypotheses evaluated and the minimal cuts found.
func (n *Neo4J) MinLabelCuts(iters []uint, cond string, candLabels []uint32, maxSize uint, minRuns uint, sinksOnly bool) ([]*LabelCut, [9]uint64, error) {
	var stats [9]uint64
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	cand := make([]C.uint32_t, len(candLabels)+1) // never empty: &cand[0] below
	for i, l := range candLabels {
		cand[i] = C.uint32_t(l)
	}
	var flags C.uint32_t
	if sinksOnly {
		flags = C.NEMO_KL_SINKS
	}
	if err := n.err(C.nemo_min_label_cuts(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), &cand[0], C.size_t(len(candLabels)), C.uint32_t(maxSize), C.uint32_t(minRuns), flags)); err != nil {
		return nil, stats, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_min_label_cuts(n.ctx, nil, nil, 0, &cnt)); err != nil {
		return nil, stats, err
	}
	rows, nLost := make([]C.nemo_label_cut, cnt+1), make([]C.uint32_t, cnt+1)
	if err := n.err(C.nemo_fetch_min_label_cuts(n.ctx, &rows[0], &nLost[0], cnt, &cnt)); err != nil {
		return nil, stats, err
	}
	if err := n.err(C.nemo_fetch_min_label_cut_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, stats, err
	}
	res := make([]*LabelCut, cnt)
	for k, lc := range rows[:cnt] {
		m := &LabelCut{NLost: uint32(nLost[k])}
		for j := 0; j < int(lc.size); j++ {
			m.Labels = append(m.Labels, uint32(lc.label[j]))
		}
		res[k] = m
	}
	return res, stats, nil
}

// GroupCut is one minimal cut over fault events: a smallest set of candidate
// groups whose joint loss defeats the outcome on at least the asked number of
// listed runs.
type GroupCut struct {
	Groups []uint32 // positions in the group list, ascending
	NLost  uint32   // the listed runs it breaks (a run listed twice counts twice)
}

// MinGroupCuts is MinLabelCuts with groups of labels as candidates
// (nemo_min_group_cuts): a fault event that removes many clock goals at once,
// such as the crash of a node, is one candidate, so "one crash plus one
// omission" is a pair.  Among the groups it returns every minimal set of at
// most maxSize (1..3) candidates whose loss together defeats the outcome on at
// least minRuns of the listed runs' pre or post provenance (0: on every one of
// them).  Minimality is over the positions in the group list.  The cuts come
// sorted by size, then by the colex rank of their positions in the list of live
// candidates.  The second result holds, per size 1..3, the live candidates
// entering the round, the hypotheses evaluated and the minimal cuts found.
func (n *Neo4J) MinGroupCuts(iters []uint, cond string, groups [][]uint32, maxSize uint, minRuns uint, sinksOnly bool) ([]*GroupCut, [9]uint64, error) {
	var stats [9]uint64
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	off := make([]C.uint64_t, len(groups)+1)
	var labels []C.uint32_t
	for k, group := range groups {
		for _, l := range group {
			labels = append(labels, C.uint32_t(l))
		}
		off[k+1] = C.uint64_t(len(labels))
	}
	labels = append(labels, 0) // never empty: &labels[0] below
	var flags C.uint32_t
	if sinksOnly {
		flags = C.NEMO_KL_SINKS
	}
	if err := n.err(C.nemo_min_group_cuts(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), &off[0], &labels[0], C.size_t(len(groups)), C.uint32_t(maxSize), C.uint32_t(minRuns), flags)); err != nil {
		return nil, stats, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_min_group_cuts(n.ctx, nil, nil, 0, &cnt)); err != nil {
		return nil, stats, err
	}
	rows, nLost := make([]C.nemo_group_cut, cnt+1), make([]C.uint32_t, cnt+1)
	if err := n.err(C.nemo_fetch_min_group_cuts(n.ctx, &rows[0], &nLost[0], cnt, &cnt)); err != nil {
		return nil, stats, err
	}
	if err := n.err(C.nemo_fetch_min_group_cut_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, stats, err
	}
	res := make([]*GroupCut, cnt)
	for k, gc := range rows[:cnt] {
		m := &GroupCut{NLost: uint32(nLost[k])}
		for j := 0; j < int(gc.size); j++ {
			m.Groups = append(m.Groups, uint32(gc.group[j]))
		}
		res[k] = m
	}
	return res, stats, nil
}

// LineageGroupCuts answers MinGroupCuts' question for sets of up to eight fault
// events (nemo_lineage_group_cuts): every minimal set of at most maxSize (1..8)
// of the groups whose loss together defeats the outcome on at least minRuns of
// the listed runs' pre or post provenance (0: on every one of them).  It
// searches the way LineageCuts does: a set that is no cut is extended only by
// events that a surviving derivation of some listed run rests on.  The cuts
// come sorted by size, then by the colex order of their positions in the group
// list; up to size 3 they are MinGroupCuts' own.  The second result holds, per
// size 0..8, the sets evaluated and the minimal cuts found.
func (n *Neo4J) LineageGroupCuts(iters []uint, cond string, groups [][]uint32, maxSize uint, minRuns uint, sinksOnly bool) ([]*GroupCut, [18]uint64, error) {
	var stats [18]uint64
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	off := make([]C.uint64_t, len(groups)+1)
	var labels []C.uint32_t
	for k, group := range groups {
		for _, l := range group {
			labels = append(labels, C.uint32_t(l))
		}
		off[k+1] = C.uint64_t(len(labels))
	}
	labels = append(labels, 0) // never empty: &labels[0] below
	var flags C.uint32_t
	if sinksOnly {
		flags = C.NEMO_KL_SINKS
	}
	if err := n.err(C.nemo_lineage_group_cuts(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), &off[0], &labels[0], C.size_t(len(groups)), C.uint32_t(maxSize), C.uint32_t(minRuns), flags)); err != nil {
		return nil, stats, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_lineage_group_cuts(n.ctx, nil, nil, 0, &cnt)); err != nil {
		return nil, stats, err
	}
	rows, nLost := make([]C.nemo_lineage_group_cut, cnt+1), make([]C.uint32_t, cnt+1)
	if err := n.err(C.nemo_fetch_lineage_group_cuts(n.ctx, &rows[0], &nLost[0], cnt, &cnt)); err != nil {
		return nil, stats, err
	}
	if err := n.err(C.nemo_fetch_lineage_group_cut_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, stats, err
	}
	res := make([]*GroupCut, cnt)
	for k, gc := range rows[:cnt] {
		m := &GroupCut{NLost: uint32(nLost[k])}
		for j := 0; j < int(gc.size); j++ {
			m.Groups = append(m.Groups, uint32(gc.group[j]))
		}
		res[k] = m
	}
	return res, stats, nil
}

// Witness is the surviving derivation of one graph under one fault hypothesis:
// what is left of the outcome's provenance, and what it rests on.
type Witness struct {
	Graph      uint32  // 2*run + cond
	Roots      uint32  // nodes of in-degree 0
	RootsAlive uint32  // 0: the hypothesis defeats the outcome and the witness is empty
	Nodes      uint32  // nodes of the witness
	Sinks      uint32  // sink goals of the witness: the base events it rests on
	Mask       []uint8 // withMasks: one byte per node of the graph, 1 = in the witness
}

func witnessFlags(all, withMasks bool) C.uint32_t {
	var flags C.uint32_t
	if all {
		flags |= C.NEMO_WIT_ALL
	}
	if withMasks {
		flags |= C.NEMO_WIT_MASKS
	}
	return flags
}

// witnessRows fetches the rows of the last witness call and, withMasks, every
// hypothesis' mask; nodes(graph) is the node count of a graph.
func (n *Neo4J) witnessRows(withMasks bool, nodes func(uint32) uint64) ([]*Witness, error) {
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_witness(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	rows := make([]C.nemo_witness, cnt+1)
	if err := n.err(C.nemo_fetch_witness(n.ctx, &rows[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	res := make([]*Witness, cnt)
	for h, w := range rows[:cnt] {
		m := &Witness{Graph: uint32(w.graph), Roots: uint32(w.n_roots), RootsAlive: uint32(w.roots_alive), Nodes: uint32(w.n_nodes), Sinks: uint32(w.n_sinks)}
		if withMasks {
			m.Mask = make([]uint8, nodes(m.Graph)+1)
			if err := n.err(C.nemo_fetch_witness_mask(n.ctx, C.uint64_t(h), (*C.uint8_t)(unsafe.Pointer(&m.Mask[0])), C.uint64_t(len(m.Mask)))); err != nil {
				return nil, err
			}
			m.Mask = m.Mask[:len(m.Mask)-1]
		}
		res[h] = m
	}
	return res, nil
}

// WitnessSets answers what a fault hypothesis that is no cut leaves behind
// (nemo_witness_sets): for every set of graph-local nodes removed from one
// run's pre or post provenance, one derivation of every surviving root (all:
// every surviving derivation) and the base events it rests on, which are the
// events the next hypothesis must hit.  nodes is the graph's node count (for
// the masks).
func (n *Neo4J) WitnessSets(iter uint, cond string, sets [][]uint32, all bool, withMasks bool, nodes uint64) ([]*Witness, error) {
	off := make([]C.uint64_t, len(sets)+1)
	var ent []C.uint32_t
	for k, set := range sets {
		for _, v := range set {
			ent = append(ent, C.uint32_t(v))
		}
		off[k+1] = C.uint64_t(len(ent))
	}
	ent = append(ent, 0) // never empty: &ent[0] below
	if err := n.err(C.nemo_witness_sets(n.ctx, C.uint32_t(iter), condIndex(cond), &off[0], &ent[0], C.size_t(len(sets)), witnessFlags(all, withMasks))); err != nil {
		return nil, err
	}
	return n.witnessRows(withMasks, func(uint32) uint64 { return nodes })
}

// WitnessLabels is WitnessSets with hypotheses that name interned labels,
// against every listed run at once (nemo_witness_labels): row i*len(sets)+s is
// set s on listed run i.  nodes(graph) is the node count of graph 2*run+cond
// (for the masks; may be nil without them).
func (n *Neo4J) WitnessLabels(iters []uint, cond string, sets [][]uint32, all bool, withMasks bool, sinksOnly bool, nodes func(uint32) uint64) ([]*Witness, error) {
	its := make([]C.uint32_t, len(iters)+1)
	for i, it := range iters {
		its[i] = C.uint32_t(it)
	}
	off := make([]C.uint64_t, len(sets)+1)
	var labels []C.uint32_t
	for k, set := range sets {
		for _, l := range set {
			labels = append(labels, C.uint32_t(l))
		}
		off[k+1] = C.uint64_t(len(labels))
	}
	labels = append(labels, 0) // never empty: &labels[0] below
	flags := witnessFlags(all, withMasks)
	if sinksOnly {
		flags |= C.NEMO_WIT_SINKS
	}
	if err := n.err(C.nemo_witness_labels(n.ctx, &its[0], C.size_t(len(iters)), condIndex(cond), &off[0], &labels[0], C.size_t(len(sets)), flags)); err != nil {
		return nil, err
	}
	return n.witnessRows(withMasks, nodes)
}

// MinRepair is one minimal repair of a failed run against a good one: a smallest
// set of base events the good run has and the failed run lacks whose presence
// would have been enough for the good run's outcome to be derived.
type MinRepair struct {
	Nodes  []uint32 // local node indices of the base run's post graph, in candidate-list order
	IDs    []string // their node IDs
	Labels []string // ... and labels
}

// RepairResult is what MinRepairs returns beside the repairs.
type RepairResult struct {
	Status     uint64    // C.NEMO_REPAIR_HOLDS, C.NEMO_REPAIR_SEARCHED or C.NEMO_REPAIR_BEYOND
	Absent     uint64    // how many base events of the base run the other run lacks
	Stats      [9]uint64 // per size 1..3: live candidates entering the round, hypotheses evaluated, minimal repairs found
	Candidates []uint32  // the absent sink goals, in node-index order
	Repairs    []*MinRepair
}

// MinRepairs returns all minimal repairs of at most maxSize (1..3) base events
// of run base's post provenance against run other (nemo_min_repairs): the
// absent set and the candidates are the sink goals of base's post graph whose
// label is no goal label of other's post graph.  It is the exact answer to the
// question the reference's missing-events heuristic approximates: which of the
// missing events, had they happened, suffice together.  Status
// C.NEMO_REPAIR_HOLDS means the absent events do not explain a failure, and
// C.NEMO_REPAIR_BEYOND cannot occur here (every absent node is a candidate);
// the repairs come sorted by size, then by the colex rank of their positions in
// the list of candidates that are no repair alone.
func (n *Neo4J) MinRepairs(base, other uint, maxSize uint) (*RepairResult, error) {
	if err := n.err(C.nemo_min_repairs(n.ctx, C.uint32_t(base), C.uint32_t(other), C.uint32_t(maxSize), 0)); err != nil {
		return nil, err
	}
	var stats [11]uint64
	if err := n.err(C.nemo_fetch_min_repair_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, err
	}
	res := &RepairResult{Status: stats[0], Absent: stats[1]}
	copy(res.Stats[:], stats[2:])
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_min_repair_cands(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	cands := make([]C.uint32_t, cnt+1) // never empty: &cands[0] below
	if err := n.err(C.nemo_fetch_min_repair_cands(n.ctx, &cands[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	for _, v := range cands[:cnt] {
		res.Candidates = append(res.Candidates, uint32(v))
	}
	if err := n.err(C.nemo_fetch_min_repairs(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	reps := make([]C.nemo_repair, cnt+1)
	if err := n.err(C.nemo_fetch_min_repairs(n.ctx, &reps[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	p := n.graphs[2*n.runIdx[base]+1]
	for _, rep := range reps[:cnt] {
		m := &MinRepair{}
		for j := 0; j < int(rep.size); j++ {
			v := uint32(rep.node[j])
			id, label := "", ""
			if int(v) < len(p.goals) {
				id, label = p.goals[v].ID, p.goals[v].Label
			}
			m.Nodes, m.IDs, m.Labels = append(m.Nodes, v), append(m.IDs, id), append(m.Labels, label)
		}
		res.Repairs = append(res.Repairs, m)
	}
	return res, nil
}

// LineageRepairResult is what LineageRepairs and LineageRepairSets return.
type LineageRepairResult struct {
	Status     uint64     // C.NEMO_REPAIR_HOLDS, C.NEMO_REPAIR_SEARCHED or C.NEMO_REPAIR_BEYOND
	Absent     uint64     // the size of the absent set
	Stats      [18]uint64 // per size 0..8: sets evaluated, minimal repairs found
	Candidates []uint32   // candidate position -> node
	Repairs    []*MinRepair
}

// lineageRepairResult fetches the result of the last lineage repair call on
// the graph p (stats, candidates, rows).
func (n *Neo4J) lineageRepairResult(p *provGraph) (*LineageRepairResult, error) {
	var stats [20]uint64
	if err := n.err(C.nemo_fetch_lineage_repair_stats(n.ctx, (*C.uint64_t)(unsafe.Pointer(&stats[0])))); err != nil {
		return nil, err
	}
	res := &LineageRepairResult{Status: stats[0], Absent: stats[1]}
	copy(res.Stats[:], stats[2:])
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_lineage_repair_cands(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	cands := make([]C.uint32_t, cnt+1) // never empty: &cands[0] below
	if err := n.err(C.nemo_fetch_lineage_repair_cands(n.ctx, &cands[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	for _, v := range cands[:cnt] {
		res.Candidates = append(res.Candidates, uint32(v))
	}
	if err := n.err(C.nemo_fetch_lineage_repairs(n.ctx, nil, 0, &cnt)); err != nil {
		return nil, err
	}
	reps := make([]C.nemo_lineage_repair, cnt+1)
	if err := n.err(C.nemo_fetch_lineage_repairs(n.ctx, &reps[0], cnt, &cnt)); err != nil {
		return nil, err
	}
	for _, rep := range reps[:cnt] {
		m := &MinRepair{}
		for j := 0; j < int(rep.size); j++ {
			v := uint32(rep.node[j])
			id, label := "", ""
			if int(v) < len(p.goals) {
				id, label = p.goals[v].ID, p.goals[v].Label
			}
			m.Nodes, m.IDs, m.Labels = append(m.Nodes, v), append(m.IDs, id), append(m.Labels, label)
		}
		res.Repairs = append(res.Repairs, m)
	}
	return res, nil
}

// LineageRepairs returns all minimal repairs of at most maxSize (1..8) base
// events of run base's post provenance against run other
// (nemo_lineage_repairs), as MinRepairs does up to size 3, by the dual of the
// search LineageCuts makes: a restore set that does not bring the outcome back
// is extended only by the missing events that lie in its blocker, the proof
// that every root is still dead.  The repairs come sorted by size, then by the
// colex order of their positions in the candidate list.
func (n *Neo4J) LineageRepairs(base, other uint, maxSize uint) (*LineageRepairResult, error) {
	if err := n.err(C.nemo_lineage_repairs(n.ctx, C.uint32_t(base), C.uint32_t(other), C.uint32_t(maxSize), 0)); err != nil {
		return nil, err
	}
	return n.lineageRepairResult(n.graphs[2*n.runIdx[base]+1])
}

// LineageRepairSets is LineageRepairs over an absent set and candidates the
// caller names, local node indices of one run's pre or post provenance
// (nemo_lineage_repair_sets); candidates nil means the absent list itself.
func (n *Neo4J) LineageRepairSets(iter uint, cond string, absent []uint32, candidates []uint32, maxSize uint) (*LineageRepairResult, error) {
	lost := make([]C.uint32_t, len(absent)+1) // never empty: &lost[0] below
	for i, v := range absent {
		lost[i] = C.uint32_t(v)
	}
	var list *C.uint32_t
	if candidates != nil {
		nodes := make([]C.uint32_t, len(candidates)+1)
		for i, v := range candidates {
			nodes[i] = C.uint32_t(v)
		}
		list = &nodes[0]
	}
	if err := n.err(C.nemo_lineage_repair_sets(n.ctx, C.uint32_t(iter), condIndex(cond), &lost[0], C.size_t(len(absent)), list, C.size_t(len(candidates)), C.uint32_t(maxSize), 0)); err != nil {
		return nil, err
	}
	return n.lineageRepairResult(n.graphs[2*n.runIdx[iter]+int(condIndex(cond))])
}

// FailureClass is one distinct failure mode among the failed runs: the runs
// whose differential provenance against the good run is the same graph.
type FailureClass struct {
	Representative uint          // iteration of the class's first failed run
	Members        []uint        // iterations of every member, in failedRuns order
	Nodes          uint          // nodes of the differential provenance
	Missing        []*fi.Missing // the representative's missing events
	Diff           *gographviz.Graph
}

// FailureClasses has no reference counterpart: it summarises what
// CreateNaiveDiffProv (differential-provenance.go:18-146) returns per failed run.
// The library groups the diff entries by identical D mask on the device
// (nemo_diff_classes); the missing events and the diff DOT are then built once
// per class, for its representative, by CreateNaiveDiffProv.  Largest class
// first, ties by representative.  Support[v] counts the failed runs whose
// differential provenance holds node v of the good run's post graph.
func (n *Neo4J) FailureClasses(failedRuns []uint, successPostProv *gographviz.Graph) ([]*FailureClass, []uint32, error) {
	f := make([]C.uint32_t, len(failedRuns)+1)
	for i, it := range failedRuns {
		f[i] = C.uint32_t(it)
	}
	if err := n.err(C.nemo_diffprov(n.ctx, &f[0], C.size_t(len(failedRuns)), C.NEMO_DIFF_REFERENCE)); err != nil {
		return nil, nil, err
	}
	if err := n.err(C.nemo_diff_classes(n.ctx)); err != nil {
		return nil, nil, err
	}
	var cnt C.uint64_t
	if err := n.err(C.nemo_fetch_diff_classes(n.ctx, nil, nil, 0, &cnt)); err != nil {
		return nil, nil, err
	}
	classOf := make([]C.uint32_t, len(failedRuns)+1)
	classes := make([]C.nemo_diff_class, cnt+1)
	if err := n.err(C.nemo_fetch_diff_classes(n.ctx, &classOf[0], &classes[0], cnt, &cnt)); err != nil {
		return nil, nil, err
	}
	V0 := n.graphs[2*n.runIdx[0]+1].n()
	sup := make([]C.uint32_t, V0+1)
	if err := n.err(C.nemo_fetch_diff_support(n.ctx, &sup[0], C.uint64_t(V0))); err != nil {
		return nil, nil, err
	}
	support := make([]uint32, V0)
	for v := range support {
		support[v] = uint32(sup[v])
	}
	out := make([]*FailureClass, cnt)
	for k := range out {
		dc := classes[k]
		out[k] = &FailureClass{Representative: failedRuns[dc.rep], Nodes: uint(dc.nodes)}
	}
	for e, it := range failedRuns {
		if len(out) > 0 {
			out[classOf[e]].Members = append(out[classOf[e]].Members, it)
		}
	}
	sort.SliceStable(out, func(a, b int) bool { return len(out[a].Members) > len(out[b].Members) })
	reps := make([]uint, len(out))
	for k, fc := range out {
		reps[k] = fc.Representative
	}
	diffs, _, missing, err := n.CreateNaiveDiffProv(false, reps, successPostProv)
	if err != nil {
		return nil, nil, err
	}
	for k, fc := range out {
		fc.Diff, fc.Missing = diffs[k], missing[k]
	}
	return out, support, nil
}

func (n *Neo4J) childrenOf(g int) map[uint32][]uint32 {
	s, d := n.graphs[g].src, n.graphs[g].dst
	ch := map[uint32][]uint32{}
	for i := range s {
		ch[s[i]] = append(ch[s[i]], d[i])
	}
	for k := range ch {
		sort.Slice(ch[k], func(a, b int) bool { return ch[k][a] < ch[k][b] })
	}
	return ch
}

func goalOf(nd graph.Node) *fi.Goal {
	p := nd.Properties
	return &fi.Goal{ID: p["id"].(string), Label: p["label"].(string), Table: p["table"].(string),
		Time: p["time"].(string), CondHolds: p["condition_holds"] == true}
}

func ruleOf(nd graph.Node) *fi.Rule {
	p := nd.Properties
	return &fi.Rule{ID: p["id"].(string), Label: p["label"].(string), Table: p["table"].(string),
		Type: p["type"].(string)}
}

// ---- corrections.go / extensions.go ---------------------------------------------------

type triggerRows struct {
	pre   [][3]uint32 // (a, g, r) of findPreTriggers (corrections.go:30-34)
	post  [][2]uint32 // (g, r) of findPostTriggers (:121-125)
	async []uint32    // async rules of GenerateExtensions (extensions.go:63-67)
}

func (n *Neo4J) triggers() (*triggerRows, error) {
	if err := n.err(C.nemo_triggers(n.ctx)); err != nil {
		return nil, err
	}
	var np, nq, na C.uint64_t
	if err := n.err(C.nemo_fetch_triggers(n.ctx, nil, 0, &np, nil, 0, &nq, nil, 0, &na)); err != nil {
		return nil, err
	}
	pre, post, asy := make([]C.uint32_t, 3*np+1), make([]C.uint32_t, 2*nq+1), make([]C.uint32_t, na+1)
	if err := n.err(C.nemo_fetch_triggers(n.ctx, &pre[0], np, &np, &post[0], nq, &nq, &asy[0], na, &na)); err != nil {
		return nil, err
	}
	t := &triggerRows{}
	for i := 0; i < int(np); i++ {
		t.pre = append(t.pre, [3]uint32{uint32(pre[3*i]), uint32(pre[3*i+1]), uint32(pre[3*i+2])})
	}
	for i := 0; i < int(nq); i++ {
		t.post = append(t.post, [2]uint32{uint32(post[2*i]), uint32(post[2*i+1])})
	}
	for i := 0; i < int(na); i++ {
		t.async = append(t.async, uint32(asy[i]))
	}
	return t, nil
}

// receiver: strings.TrimLeft(label, table) -- a cutset trim -- then Trim "()"
// and the first ", " field (corrections.go:65-67,155-157).
func receiver(label, table string) string {
	return strings.Split(strings.Trim(strings.TrimLeft(label, table), "()"), ", ")[0]
}

// GenerateCorrections (corrections.go:202-328): the trigger rows of run 0 come
// from the device; the maps findPreTriggers / findPostTriggers returned are
// rebuilt with one fresh key per row (:76,168) and fed to the reference's own
// string synthesis (:219-324, kept verbatim as synthesizeCorrections).
func (n *Neo4J) GenerateCorrections() ([]string, error) {
	t, err := n.triggers()
	if err != nil {
		return nil, err
	}
	r0 := n.runIdx[0]
	gp, gq := 2*r0, 2*r0+1
	flp, err := n.flags(gp)
	if err != nil {
		return nil, err
	}
	flq, err := n.flags(gq)
	if err != nil {
		return nil, err
	}
	preTriggers := map[*fi.Rule][]*GoalRulePair{}
	for _, row := range t.pre {
		goal := goalOf(n.node(gp, row[1], flp, nil))
		goal.Receiver = receiver(goal.Label, goal.Table)
		agg := ruleOf(n.node(gp, row[0], flp, nil))
		preTriggers[agg] = append(preTriggers[agg], &GoalRulePair{Goal: goal, Rule: ruleOf(n.node(gp, row[2], flp, nil))})
	}
	postTriggers := map[*fi.Goal][]*fi.Rule{}
	for _, row := range t.post {
		goal := goalOf(n.node(gq, row[0], flq, nil))
		goal.Receiver = receiver(goal.Label, goal.Table)
		postTriggers[goal] = append(postTriggers[goal], ruleOf(n.node(gq, row[1], flq, nil)))
	}
	return synthesizeCorrections(preTriggers, postTriggers), nil
}

// GenerateExtensions (extensions.go:13-99): the holding-"pre" goal count is
// entry 2T+2 of the reduction vector (every shard's count summed);
// allAchievedPre = !(count < len(Runs)) (:47-49).
func (n *Neo4J) GenerateExtensions() (bool, []string, error) {
	red := n.red
	if red == nil {
		var err error
		if red, err = n.reduce(nil); err != nil {
			return false, nil, err
		}
	}
	if !(red.preHolds < uint64(len(n.Runs))) {
		return true, nil, nil
	}
	t, err := n.triggers()
	if err != nil {
		return false, nil, err
	}
	gp := 2 * n.runIdx[0]
	fl, err := n.flags(gp)
	if err != nil {
		return false, nil, err
	}
	state := map[string]string{}
	for _, r := range t.async { // one suggestion per distinct table (:83-90)
		table := n.node(gp, r, fl, nil).Properties["table"].(string)
		state[table] = fmt.Sprintf("<code>%s(node, ...)@async :- ...;</code>", table)
	}
	ext := make([]string, 0, len(state))
	for _, s := range state {
		ext = append(ext, s)
	}
	return false, ext, nil
}
