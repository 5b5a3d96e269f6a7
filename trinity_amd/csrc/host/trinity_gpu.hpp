// trinity_gpu.hpp — host-side C++ operator surface of the MI355X engine.
//
// Keeps the shape of Trinity's classes on the hot path so application code written against the reference reads
// the same here:  Codecs::{AccessProxy, Decoder, PostingsListIterator}  (codecs.h:211-317),
// DocsSetIterators::{Iterator, Conjuction, Disjunction, …}  (docset_iterators_base.h:45-96, docset_iterators.h),
// relevant_document_provider / IteratorScorer  (relevant_documents.h:22-81),  MatchesProxy + DocsSetSpan
// (docset_spans.h:14-90),  Similarity::{ScorerWeight, IndexSourceTermsScorer, IndexSourcesCollectionBM25Scorer}
// (similarity.h:22-255),  MatchedIndexDocumentsFilter (matches.h:139-185),  IndexSource (index_source.h:19-156),
// ExecFlags + exec_query (exec.h:11-52).
//
// What is different underneath: nothing here walks postings on the CPU.  An Iterator is a *plan node*; the first
// next()/advance() (or a span's process()) lowers the tree to a postfix program, runs it through the C-ABI
// (include/trinity_hip.h) on the GPU and then walks the materialised result.  Errors from the C-ABI surface as the
// exception type the reference would have thrown at that point.  New code — no reference source.
#pragma once
#include "../../../include/trinity_hip.h"
#include "google_encoder.hpp"
#include "facet_rows.hpp"
#include "order_rows.hpp"
#include "stats_rows.hpp"
#include "column_pred.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace trinity_amd {
        using isrc_docid_t = uint32_t; // common.h:36
        using docid_t = uint32_t;      // common.h:39
        using tokenpos_t = uint16_t;   // common.h:46
        using exec_term_id_t = uint16_t; // common.h: per-query term id
        static constexpr isrc_docid_t DocIDsEND{std::numeric_limits<isrc_docid_t>::max()}; // common.h:43

        enum class ExecFlags : uint32_t { DocumentsOnly = 1, AccumulatedScoreScheme = 2 }; // exec.h:11-43

        // Switch::{invalid_argument, data_error, system_error} stand-ins (Switch/switch_exceptions.h)
        struct invalid_argument : std::invalid_argument { using std::invalid_argument::invalid_argument; };
        struct data_error : std::runtime_error { using std::runtime_error::runtime_error; };
        struct system_error : std::runtime_error { using std::runtime_error::runtime_error; };
        struct aborted_search_exception final : std::exception { // matches.h:132-137
                const char *what() const noexcept override { return "Search Aborted"; }
        };

        inline void check(int rc) {
                if (rc == TRI_OK)
                        return;
                const std::string msg = tri_last_error();
                switch (rc) {
                        case TRI_ERR_INVALID:
                        case TRI_ERR_UNSUPPORTED:
                                throw invalid_argument(msg);
                        case TRI_ERR_FORMAT:
                                throw data_error(msg);
                        default:
                                throw system_error(msg);
                }
        }

        // ------------------------------------------------------------------ relevant documents / scorers
        struct relevant_document_provider { // relevant_documents.h:22-41
                virtual isrc_docid_t document() const noexcept = 0;
                inline double score();
                virtual ~relevant_document_provider() = default;
        };

        namespace DocsSetIterators {
                struct Iterator;
        }

        struct IteratorScorer : public relevant_document_provider { // relevant_documents.h:48-72
                DocsSetIterators::Iterator *const it;
                explicit IteratorScorer(DocsSetIterators::Iterator *i)
                    : it{i} {}
                inline isrc_docid_t document() const noexcept override;
                virtual double iterator_score() = 0;
        };

        inline double relevant_document_provider::score() { return static_cast<IteratorScorer *>(this)->iterator_score(); }

        class IndexSource;

        namespace Similarity { // similarity.h
                struct ScorerWeight {
                        virtual ~ScorerWeight() = default;
                };
                struct IndexSourcesCollectionTermsScorer;
                struct IndexSourceTermsScorer {
                        IndexSource *const src;
                        IndexSourcesCollectionTermsScorer *const collectionScorer;
                        IndexSourceTermsScorer(IndexSourcesCollectionTermsScorer *r, IndexSource *s)
                            : src{s}, collectionScorer{r} {}
                        virtual ~IndexSourceTermsScorer() = default;
                        virtual ScorerWeight *new_scorer_weight(const std::string *terms, uint16_t cnt) = 0;
                        virtual float score(isrc_docid_t id, uint16_t freq, const ScorerWeight *) = 0;
                        // the engine evaluates score() on the device: the scorer says which device formula it is and
                        // what per-term weight to feed it
                        virtual int device_similarity() const = 0;
                        virtual double device_weight(const ScorerWeight *) const = 0;
                };
                struct IndexSourcesCollectionTermsScorer {
                        virtual ~IndexSourcesCollectionTermsScorer() = default;
                        virtual IndexSourceTermsScorer *new_source_scorer(IndexSource *) = 0;
                };
        } // namespace Similarity

        // ------------------------------------------------------------------ iterators (plan nodes + cursors)
        namespace DocsSetIterators {
                enum class Type : uint8_t { PostingsListIterator = 0, DisjunctionSome = 1, Filter = 2, Optional = 3, Disjunction = 4, DisjunctionAllPLI, Phrase, Conjuction, ConjuctionAllPLI }; // docset_iterators_base.h:10-23

                struct Iterator : public relevant_document_provider { // docset_iterators_base.h:45-96
                        struct {
                                isrc_docid_t id{0};
                        } curDocument;
                        const Type type;
                        IndexSource *const isrc;

                        Iterator(Type t, IndexSource *s)
                            : type{t}, isrc{s} {}
                        inline isrc_docid_t current() const noexcept { return curDocument.id; }
                        isrc_docid_t document() const noexcept override { return curDocument.id; }

                        // first document > current (DocIDsEND when exhausted)
                        isrc_docid_t next() {
                                materialize();
                                return curDocument.id = cursor < docs.size() ? docs[cursor++] : DocIDsEND;
                        }
                        // first document >= target (may stay on the current one, docset_iterators_base.h:73-80)
                        isrc_docid_t advance(const isrc_docid_t target) {
                                materialize();
                                if (curDocument.id != 0 && curDocument.id >= target)
                                        return curDocument.id;
                                size_t lo = cursor, hi = docs.size();
                                while (lo < hi) {
                                        const size_t mid = (lo + hi) / 2;
                                        if (docs[mid] < target)
                                                lo = mid + 1;
                                        else
                                                hi = mid;
                                }
                                cursor = lo;
                                return next();
                        }
                        virtual uint64_t cost() const = 0; // docset_iterators.cpp:10-64
                        // emit this subtree as postfix tokens; `w` (parallel to prog) receives each TERM token's ScorerWeight
                        virtual void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const = 0;

                      protected:
                        std::vector<isrc_docid_t> docs;
                        size_t cursor{0};
                        bool materialized{false};
                        virtual void materialize(); // default: run this subtree as one DocumentsOnly query on the GPU
                        friend class ::trinity_amd::IndexSource;
                };
        } // namespace DocsSetIterators

        inline isrc_docid_t IteratorScorer::document() const noexcept { return it->current(); }

        // ------------------------------------------------------------------ positions scratch
        // docwordspace.h:16-92, restated: which query term sits at each position of the CURRENT document.  ONE term per position — set() replaces whatever
        // was there, the last writer wins —, test(term, pos) asks "is it this term", reset() forgets the document in O(1): a cell carries the sequence number
        // of the document that wrote it and counts only while that is the current one (every 65 535 resets the cells are cleared and the numbers start
        // again at 1).  Position 0 means "no position" in the index and is never set (the callers skip it: materialize_hits).  The reference sizes the space
        // by the largest indexed position and leaves a set() past it to the caller's care; here every tokenpos_t is a valid cell (and MaxPhraseSize more, so
        // that a phrase test may run past the last position without a bound check)
        class DocWordsSpace final {
                static constexpr uint32_t MaxPhraseSize = 16; // trinity_limits.h:12
                std::vector<uint32_t> cells;                   // termID << 16 | sequence number of the writing document (0: never written)
                const uint32_t maxPos;
                uint16_t curSeq{1};

              public:
                explicit DocWordsSpace(const uint32_t max = 16383) // trinity_limits.h:15 MaxPosition
                    : cells(size_t(std::numeric_limits<tokenpos_t>::max()) + 1 + MaxPhraseSize, 0u), maxPos{max} {
                        if (!max || max > std::numeric_limits<tokenpos_t>::max())
                                throw invalid_argument("DocWordsSpace: max position out of range");
                }
                void reset() {
                        if (curSeq == std::numeric_limits<uint16_t>::max()) {
                                std::fill(cells.begin(), cells.end(), 0u);
                                curSeq = 1;
                        } else
                                ++curSeq;
                }
                void set(const exec_term_id_t termID, const tokenpos_t pos) noexcept { cells[pos] = uint32_t(termID) << 16 | curSeq; }
                bool test(const exec_term_id_t termID, const uint32_t pos) const noexcept { return pos < cells.size() && cells[pos] == (uint32_t(termID) << 16 | curSeq); }
                void unset(const tokenpos_t pos) noexcept { cells[pos] = 0; }
                uint32_t max_pos() const noexcept { return maxPos; }
        };
        struct term_hit;

        // ------------------------------------------------------------------ codecs
        namespace Codecs { // codecs.h:211-317
                struct Decoder;
                struct PostingsListIterator : public DocsSetIterators::Iterator {
                        Decoder *const dec;
                        tokenpos_t freq{0};
                        inline PostingsListIterator(Decoder *d);
                        inline isrc_docid_t next() {
                                const auto id = Iterator::next();
                                freq = id == DocIDsEND ? 0 : tokenpos_t(freqs[cursor - 1]);
                                return id;
                        }
                        inline isrc_docid_t advance(isrc_docid_t target) {
                                const auto id = Iterator::advance(target);
                                freq = id == DocIDsEND ? 0 : tokenpos_t(freqs[cursor - 1]);
                                return id;
                        }
                        Decoder *decoder() noexcept { return dec; }
                        uint64_t cost() const override;
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override;
                        // codecs.h:229-235: the hits of the CURRENT document into out[0 .. freq) — term_hit{payload, pos, payloadLen} — and dws->set(termID, pos) for
                        // every pos != 0 (termID = the decoder's execCtxTermID).  The first call of a list fetches all its hits ONCE from the device
                        // (tri_decode_hits); later calls copy.  Unlike the reference's it may be called again for the same document, and in any order
                        inline void materialize_hits(DocWordsSpace *dws, term_hit *out);

                      protected:
                        std::vector<uint32_t> freqs;
                        void materialize() override; // tri_decode_terms: the whole list, docIDs + freqs
                        // materialize_hits' copy of the list's hits, and where each document's begin (the running sum of the STORED frequencies)
                        bool hitsFetched{false};
                        std::vector<uint16_t> hitPos;
                        std::vector<uint8_t> hitLen;
                        std::vector<uint64_t> hitPayload, hitFirst;
                };

                struct AccessProxy;
                struct Decoder {
                        term_index_ctx indexTermCtx;
                        uint32_t termId{0}; // row of the uploaded term table
                        exec_term_id_t execCtxTermID{0}; // the query's id of the term (codecs.h Decoder::execCtxTermID): what materialize_hits sets in the DocWordsSpace
                        std::string term;
                        IndexSource *isrc{nullptr};
                        virtual ~Decoder() = default;
                        virtual void init(const term_index_ctx &, AccessProxy *) = 0;
                        virtual PostingsListIterator *new_iterator() { return new PostingsListIterator(this); }
                };

                struct AccessProxy {
                        const uint8_t *const indexPtr;
                        explicit AccessProxy(const uint8_t *p)
                            : indexPtr{p} {}
                        virtual ~AccessProxy() = default;
                        virtual Decoder *new_decoder(const term_index_ctx &) = 0;
                        virtual const char *codec_identifier() = 0;
                };

                namespace Google {
                        struct Decoder final : public Codecs::Decoder {
                                void init(const term_index_ctx &t, Codecs::AccessProxy *) override { indexTermCtx = t; }
                        };
                        struct AccessProxy final : public Codecs::AccessProxy {
                                using Codecs::AccessProxy::AccessProxy;
                                const char *codec_identifier() override { return "GOOGLE"; }
                                Codecs::Decoder *new_decoder(const term_index_ctx &t) override {
                                        auto d = new Decoder();
                                        d->init(t, this);
                                        return d;
                                }
                        };
                } // namespace Google

                // lucene_codec.h:246-283 — the codec SegmentIndexSource picks for a segment whose `id` file names "LUCENE"
                // (segment_index_source.cpp:172-179).  Besides the index it maps the segment's hits.data (lucene_codec.h:206: positions and payloads
                // live in their own file).  The engine reads this repo's PFOR128 ints() payload (include/pfor128.md), see INTEGRATION.md §1
                namespace Lucene {
                        struct Decoder final : public Codecs::Decoder {
                                void init(const term_index_ctx &t, Codecs::AccessProxy *) override { indexTermCtx = t; }
                        };
                        struct AccessProxy final : public Codecs::AccessProxy {
                                const uint8_t *const hitsDataPtr;
                                AccessProxy(const uint8_t *index, const uint8_t *hits)
                                    : Codecs::AccessProxy(index), hitsDataPtr{hits} {}
                                const char *codec_identifier() override { return "LUCENE"; }
                                Codecs::Decoder *new_decoder(const term_index_ctx &t) override {
                                        auto d = new Decoder();
                                        d->init(t, this);
                                        return d;
                                }
                        };
                } // namespace Lucene
        }         // namespace Codecs

        inline Codecs::PostingsListIterator::PostingsListIterator(Decoder *d)
            : Iterator{DocsSetIterators::Type::PostingsListIterator, d->isrc}, dec{d} {}

        // ------------------------------------------------------------------ composite iterators
        namespace DocsSetIterators {
                struct Conjuction final : public Iterator { // docset_iterators.h:333-362
                        std::vector<Iterator *> its;
                        Conjuction(Iterator **iterators, uint16_t cnt)
                            : Iterator{Type::Conjuction, iterators[0]->isrc}, its(iterators, iterators + cnt) {}
                        uint64_t cost() const override { // the cheapest member leads (exec.cpp:154-170, 44-55)
                                uint64_t c = UINT64_MAX;
                                for (auto it : its)
                                        c = std::min(c, it->cost());
                                return c;
                        }
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override {
                                for (auto it : its)
                                        it->lower(prog, w, scorer);
                                prog.push_back(TRI_TOK(TRI_OP_AND, its.size()));
                                w.push_back(0.0);
                        }
                };
                struct Disjunction final : public Iterator { // docset_iterators.h:261-303
                        std::vector<Iterator *> its;
                        Disjunction(Iterator **iterators, uint16_t cnt)
                            : Iterator{Type::Disjunction, iterators[0]->isrc}, its(iterators, iterators + cnt) {}
                        uint64_t cost() const override {
                                uint64_t c = 0;
                                for (auto it : its)
                                        c += it->cost();
                                return c;
                        }
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override {
                                for (auto it : its)
                                        it->lower(prog, w, scorer);
                                prog.push_back(TRI_TOK(TRI_OP_OR, its.size()));
                                w.push_back(0.0);
                        }
                };
                struct DisjunctionSome final : public Iterator { // docset_iterators.h:61-137 (matchsome, exec.cpp:276-283): documents at least minMatch members hold
                        std::vector<Iterator *> its;
                        const uint16_t matchThreshold;
                        DisjunctionSome(Iterator **iterators, uint16_t cnt, uint16_t minMatch)
                            : Iterator{Type::DisjunctionSome, iterators[0]->isrc}, its(iterators, iterators + cnt), matchThreshold{minMatch} {}
                        uint64_t cost() const override { // docset_iterators.cpp:733-742: the (cnt - minMatch + 1) cheapest members
                                std::vector<uint64_t> cs;
                                for (auto it : its)
                                        cs.push_back(it->cost());
                                std::sort(cs.begin(), cs.end());
                                uint64_t c = 0;
                                for (size_t i = 0; i + matchThreshold <= cs.size(); ++i)
                                        c += cs[i];
                                return c;
                        }
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override {
                                for (auto it : its)
                                        it->lower(prog, w, scorer);
                                prog.push_back(TRI_TOK(TRI_OP_SOME, (uint32_t(matchThreshold) << 16) | uint32_t(its.size())));
                                w.push_back(0.0);
                        }
                };
                struct Filter final : public Iterator { // docset_iterators.h:147-172: documents of req that filter does not hold
                        Iterator *const req, *const filter;
                        Filter(Iterator *const r, Iterator *const f)
                            : Iterator{Type::Filter, r->isrc}, req{r}, filter{f} {}
                        uint64_t cost() const override { return req->cost(); } // docset_iterators.cpp:10-64
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override {
                                req->lower(prog, w, scorer);
                                filter->lower(prog, w, nullptr); // the excluded side is never scored (docset_iterators_scorers.cpp:59-73)
                                prog.push_back(TRI_TOK(TRI_OP_NOT, 2));
                                w.push_back(0.0);
                        }
                };
                struct Optional final : public Iterator { // docset_iterators.h:174-206: main's documents; opt adds score / matched terms where it matches
                        Iterator *const main, *const opt;
                        Optional(Iterator *const m, Iterator *const o)
                            : Iterator{Type::Optional, m->isrc}, main{m}, opt{o} {}
                        uint64_t cost() const override { return main->cost(); }
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override {
                                main->lower(prog, w, scorer);
                                opt->lower(prog, w, scorer);
                                prog.push_back(TRI_TOK(TRI_OP_OPT, 2));
                                w.push_back(0.0);
                        }
                };
                struct Phrase final : public Iterator { // docset_iterators.h:364-402
                        std::vector<Codecs::PostingsListIterator *> its;
                        Phrase(Codecs::PostingsListIterator **iterators, uint16_t cnt)
                            : Iterator{Type::Phrase, iterators[0]->isrc}, its(iterators, iterators + cnt) {}
                        uint64_t cost() const override { return its[0]->cost() + UINT32_MAX + uint64_t(UINT16_MAX) * its.size(); } // exec.cpp:28-34
                        void lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const override;
                };

                // docset_iterators.h:456-497: the provider a span hands to MatchesProxy::process for a materialised match.
                // score() on a provider static_casts to IteratorScorer (relevant_documents.h:76-81), so it is one.
                struct relevant_document final : public IteratorScorer {
                        struct DummyIterator final : public Iterator {
                                DummyIterator()
                                    : Iterator{Type::PostingsListIterator, nullptr} {}
                                uint64_t cost() const override { return 0; }
                                void lower(std::vector<uint32_t> &, std::vector<double> &, Similarity::IndexSourceTermsScorer *) const override { throw invalid_argument("not a plan node"); }
                        } dummy;
                        double score_{0};
                        relevant_document()
                            : IteratorScorer{&dummy} {}
                        void set_document(const isrc_docid_t id) noexcept { dummy.curDocument.id = id; }
                        double iterator_score() override { return score_; }
                };
        } // namespace DocsSetIterators
        using DocsSetIterators::relevant_document;

        // ------------------------------------------------------------------ spans, proxies, filters
        class MatchesProxy { // docset_spans.h:14-21
              public:
                virtual void process(relevant_document_provider *) {}
                virtual ~MatchesProxy() = default;
        };

        // ---- what the default execution mode hands to the application (matches.h:34-130); it fills positions only (payload and payloadLen stay 0 there:
        //      PostingsListIterator::materialize_hits and IndexSource::term_hits_at fill all three)
        struct term_hit { // runtime.h:8-20
                uint64_t payload{0};
                tokenpos_t pos{0};
                uint8_t payloadLen{0};
        };
        struct term_hits {
                tokenpos_t freq{0};
                term_hit *all{nullptr};
        };
        struct query_term_ctx {
                struct {
                        exec_term_id_t id;
                        std::string token;
                } term;
        };
        struct matched_query_term {
                const query_term_ctx *queryCtx;
                term_hits *hits;
        };
        struct matched_document {
                docid_t id{0};
                uint16_t matchedTermsCnt{0};
                matched_query_term *matchedTerms{nullptr};
        };

        // The device form of a MatchedIndexDocumentsFilter that consumes a query's docID set (FacetCounter, ColumnOrder, StatsCounter below): a DocumentsOnly exec_query
        // binds it to the source it runs against and, when on_device() — and nothing but the device decides which documents count —, installs its spec on the batch
        // (tri_batch_set_facets / _order / _stats) and reads query q's rows of the nq back, instead of delivering the docID set and replaying consider().
        struct DeviceConsumer {
                virtual void bind(IndexSource *) = 0;
                virtual bool on_device() const = 0;
                virtual void install(tri_batch *) = 0;
                virtual void read(tri_batch *, size_t q, size_t nq) = 0;
                virtual ~DeviceConsumer() = default;
        };
        struct MatchedIndexDocumentsFilter { // matches.h:139-185
                virtual void consider(const matched_document &) {} // default execution mode
                virtual void consider(const docid_t) {}
                virtual void consider(const docid_t *ids, const size_t cnt) {
                        for (size_t i = 0; i != cnt; ++i)
                                consider(ids[i]);
                }
                virtual void consider(const docid_t, const double) {}
                // A filter whose consider(const matched_document &) is the engine's own proximity ranker (ProximityRanker below) says so here: it fills in the
                // tri_ranker and the weights of the query's terms (per matchedTerms[].queryCtx->term.id - 1) and returns where the ranked list goes; the default
                // mode's exec_query then ranks on the device (tri_batch_set_ranker) and replays no match.  nullptr (every other filter): consider() per match.
                virtual std::vector<std::pair<docid_t, double>> *device_ranker(tri_ranker *, std::vector<double> *) { return nullptr; }
                // A filter that counts, orders or aggregates its documents by per-document columns (FacetCounter, ColumnOrder, StatsCounter below) says so here: a
                // DocumentsOnly exec_query binds it to the source it runs against and, unless it asks for the replay, has the device consume the set and replays no
                // match.  nullptr: every other filter.
                virtual DeviceConsumer *device_consumer() { return nullptr; }
                virtual ~MatchedIndexDocumentsFilter() = default;
        };

        // The application-side definition of tri_batch_set_ranker's TRI_RANK_PROXIMITY score, in C++: what an application's consider(const matched_document &)
        // (matches.h:109-153) computes from matchedTerms[] (queryexec_ctx.cpp:382-648) when it ranks by capped term frequency and adjacency of consecutive
        // query terms —
        //   score = (sum over the matched terms, ascending term id: weight[id - 1] * double(min(freq, freq_cap)))
        //           + adjacency * double(hits of term id at a position p != 0 with term id + 1 at p + 1, over the ids matched together with their successor)
        // — and a K-heap under the rule score descending, docID ascending.  exec_query's default mode recognises it (device_ranker) and, with device == true, has
        // the engine compute the same list on the device; device = false keeps the per-match replay through consider(), for comparison.
        struct ProximityRanker : public MatchedIndexDocumentsFilter {
                uint32_t topk, freq_cap;
                double adjacency;
                std::vector<double> weights; // per query term, in the order of the query's terms (term.id - 1); a term past the end weighs 1.0
                bool device{true};
                std::vector<std::pair<docid_t, double>> list; // the kept matches; ranked() orders them

                explicit ProximityRanker(uint32_t k, uint32_t cap = 65535, double adj = 0.0, std::vector<double> w = {})
                    : topk{k}, freq_cap{cap}, adjacency{adj}, weights(std::move(w)) {}

                static bool better(const std::pair<docid_t, double> &a, const std::pair<docid_t, double> &b) {
                        return a.second > b.second || (a.second == b.second && a.first < b.first);
                }
                // (one rounding per operation, as the contract writes it: the products are kept out of fused multiply-adds)
                static double score_of(const matched_document &md, const std::vector<double> &weights, const uint32_t freq_cap, const double adjacency) {
                        const term_hits *by[65] = {};
                        for (uint16_t i = 0; i < md.matchedTermsCnt; ++i) {
                                const uint32_t id = md.matchedTerms[i].queryCtx->term.id;
                                if (id >= 1 && id <= 64)
                                        by[id] = md.matchedTerms[i].hits;
                        }
                        double sum = 0.0;
                        uint64_t pairs = 0;
                        for (uint32_t id = 1; id <= 64; ++id) {
                                if (!by[id])
                                        continue;
                                const double w = id - 1 < weights.size() ? weights[id - 1] : 1.0;
                                volatile double term = w * double(std::min<uint32_t>(by[id]->freq, freq_cap));
                                sum += term;
                                if (id < 64 && by[id + 1]) {
                                        const term_hits *a = by[id], *b = by[id + 1];
                                        uint32_t j = 0;
                                        for (uint32_t i = 0; i < a->freq; ++i) {
                                                const uint32_t p = a->all[i].pos;
                                                if (!p)
                                                        continue;
                                                while (j < b->freq && b->all[j].pos < p + 1u)
                                                        ++j;
                                                pairs += j < b->freq && b->all[j].pos == p + 1u;
                                        }
                                }
                        }
                        volatile double bonus = adjacency * double(pairs);
                        return sum + bonus;
                }
                void consider(const matched_document &md) override {
                        list.emplace_back(md.id, score_of(md, weights, freq_cap, adjacency));
                        std::push_heap(list.begin(), list.end(), better); // (the heap's top: the worst kept match)
                        if (list.size() > topk) {
                                std::pop_heap(list.begin(), list.end(), better);
                                list.pop_back();
                        }
                }
                std::vector<std::pair<docid_t, double>> *device_ranker(tri_ranker *spec, std::vector<double> *w) override {
                        if (!device)
                                return nullptr;
                        *spec = tri_ranker{TRI_RANK_PROXIMITY, topk, freq_cap, 0, adjacency};
                        *w = weights;
                        return &list;
                }
                // best first: score descending, docID ascending
                std::vector<std::pair<docid_t, double>> ranked() const {
                        auto out = list;
                        std::sort(out.begin(), out.end(), better);
                        return out;
                }
                // The lists of a collection's sources (exec_query's collection form, oldest source first) blended into one: the best K under score descending, docID
                // ascending, source ascending — a stable sort of the lists one after the other, so where two sources hold the same docID at the same score (no
                // masks installed) both entries stay, the older source's first.  The host form of tri_cbatch_ranked's device merge (k_rank_merge_sources).
                static std::vector<std::pair<docid_t, double>> blend(const std::vector<std::unique_ptr<ProximityRanker>> &parts, const size_t K) {
                        std::vector<std::pair<docid_t, double>> out;
                        for (const auto &p : parts) {
                                const auto l = p->ranked();
                                out.insert(out.end(), l.begin(), l.end());
                        }
                        std::stable_sort(out.begin(), out.end(), better);
                        if (out.size() > K)
                                out.resize(K);
                        return out;
                }
        };

        struct IndexDocumentsFilter { // matches.h:198-201: return true to disregard the document
                virtual bool filter(const docid_t) = 0;
                // The filter as a device bitmap (tri_filter), if it has one: exec_query / exec_queries then install it with tri_batch_set_filters and the matching
                // kernels drop its documents themselves — match counts and the engine's top-K never see them.  nullptr (every plain host filter): filter() is
                // called per replayed document, as before.
                virtual tri_filter *device_filter() { return nullptr; }
                virtual ~IndexDocumentsFilter() = default;
        };

        // ------------------------------------------------------------------ index source (GPU resident)
        struct field_statistics { // index_source.h:44-53
                uint64_t sumTermHits{0};
                uint32_t totalTerms{0};
                uint64_t sumTermsDocs{0};
                uint32_t docsCnt{0};
        };

        class IndexSource { // index_source.h:19-156, backed by an uploaded segment
                tri_dev *dev{nullptr};
                tri_index *ix{nullptr};
                std::vector<std::string> names;                 // row -> term
                std::unordered_map<std::string, uint32_t> dict; // term -> row; the reference's SegmentTerms (terms.h) is host-only and out of scope
                std::vector<term_index_ctx> table;
                std::unique_ptr<Codecs::AccessProxy> access; // Google or Lucene, by the codec name of the segment (segment_index_source.cpp:172-179)
                std::vector<std::unique_ptr<Codecs::Decoder>> decoders;
                std::vector<std::unique_ptr<DocsSetIterators::Iterator>> registry; // queryexec_ctx::reg_pli / reg_docset_it
                field_statistics fs;

                std::vector<docid_t> masked; // the set installed with set_masked_documents (kept: exec_query's per-call registry restores it)

              public:
                // `index`/`len`: the segment's raw `index` bytes; terms[i] names table[i].  `codec`: the name in the segment's `id` file — "GOOGLE", or
                // "LUCENE" with the segment's hits.data in `hits` (segment_index_source.cpp:147-179 reads the name and picks the AccessProxy)
                IndexSource(int device, const uint8_t *index, size_t len, const std::vector<std::string> &terms, const std::vector<term_index_ctx> &tctx,
                            const field_statistics &stats, const std::string &codec = "GOOGLE", const uint8_t *hits = nullptr, size_t hits_len = 0)
                    : table(tctx), fs(stats) {
                        if (terms.size() != tctx.size())
                                throw invalid_argument("terms/tctx size mismatch");
                        if (codec != "GOOGLE" && codec != "LUCENE")
                                throw invalid_argument("unknown codec"); // segment_index_source.cpp:178: "Unknown codec"
                        check(tri_dev_open(device, &dev));
                        static_assert(sizeof(term_index_ctx) == sizeof(tri_term), "term_index_ctx layout");
                        const bool lucene = codec == "LUCENE";
                        const int rc = tri_index_upload(dev, index, len, lucene ? hits : nullptr, lucene ? hits_len : 0, lucene ? TRI_CODEC_LUCENE : TRI_CODEC_GOOGLE,
                                                        reinterpret_cast<const tri_term *>(tctx.data()), tctx.size(), stats.docsCnt, &ix);
                        if (rc != TRI_OK) {
                                const std::string why = tri_last_error();
                                tri_dev_close(dev);
                                dev = nullptr;
                                throw data_error(why);
                        }
                        names = terms;
                        for (uint32_t i = 0; i < terms.size(); ++i)
                                dict.emplace(terms[i], i);
                        if (lucene)
                                access.reset(new Codecs::Lucene::AccessProxy(index, hits));
                        else
                                access.reset(new Codecs::Google::AccessProxy(index));
                }
                ~IndexSource() {
                        registry.clear();
                        tri_index_destroy(ix);
                        tri_dev_close(dev);
                }
                IndexSource(const IndexSource &) = delete;

                tri_index *handle() const noexcept { return ix; }
                // a planner / launch option of the source's device handle (tri_dev_set_option: read when a batch is created) — "rich_max_terms" = 64 lets the
                // default mode deliver matched_documents for queries of up to 64 terms
                void set_option(const char *name, const uint64_t value) { check(tri_dev_set_option(dev, name, value)); }
                const std::string &term_name(const uint32_t row) const { return names.at(row); }
                // The documents of this source that newer sources of the collection have updated or deleted — what
                // IndexSourcesCollection::commit() derives per source (index_source.cpp:3-30) and exec_query tests through
                // masked_documents_registry::test before every consider() (exec.cpp:914-975).  Uploaded once per refresh of the
                // collection; the matching kernels drop these documents themselves.
                void set_masked_documents(const std::vector<docid_t> &ids) {
                        check(tri_index_set_masked(ix, ids.data(), ids.size()));
                        masked = ids;
                }
                const std::vector<docid_t> &masked_documents() const noexcept { return masked; }
                field_statistics default_field_stats() const { return fs; }

                // index_source.h:103: unknown term => no documents
                term_index_ctx resolve_term_ctx(const std::string &term) const {
                        const auto it = dict.find(term);
                        return it == dict.end() ? term_index_ctx{} : table[it->second];
                }
                uint32_t term_id(const std::string &term) const {
                        const auto it = dict.find(term);
                        return it == dict.end() ? 0x0fffffffu : it->second; // an id past the table == "no documents" for the engine
                }
                // index_source.h:119
                Codecs::Decoder *new_postings_decoder(const std::string &term, const term_index_ctx ctx) {
                        auto d = access->new_decoder(ctx);
                        d->termId = term_id(term);
                        d->term = term;
                        d->isrc = this;
                        decoders.emplace_back(d);
                        return d;
                }

                // The hits of chosen (term, document) pairs in one engine call (tri_decode_hits_at) — what candidate_document::materialize_term_hits
                // (queryexec_ctx.cpp:317-351) asks of the codec, for a caller that holds many candidates at once.  pairs: (row of the term table, document), in
                // any order, repeats allowed.  freqs[i]: the document's stored frequency, 0xffffffff when the list does not hold it; pair i's hits are
                // hits[offsets[i] .. offsets[i + 1])
                struct pair_hits {
                        std::vector<uint32_t> freqs;
                        std::vector<uint64_t> offsets;
                        std::vector<term_hit> hits;
                };
                pair_hits term_hits_at(const std::vector<std::pair<uint32_t, isrc_docid_t>> &pairs) const {
                        std::vector<uint32_t> t(pairs.size()), d(pairs.size());
                        for (size_t i = 0; i < pairs.size(); ++i) {
                                t[i] = pairs[i].first;
                                d[i] = pairs[i].second;
                        }
                        pair_hits r;
                        r.freqs.resize(pairs.size());
                        r.offsets.resize(pairs.size() + 1);
                        check(tri_decode_hits_at(ix, t.data(), d.data(), t.size(), r.freqs.data(), nullptr, nullptr, nullptr, 0, r.offsets.data()));
                        const size_t n = size_t(r.offsets.back());
                        std::vector<uint16_t> pos(n);
                        std::vector<uint8_t> len(n);
                        std::vector<uint64_t> word(n);
                        if (n)
                                check(tri_decode_hits_at(ix, t.data(), d.data(), t.size(), r.freqs.data(), pos.data(), len.data(), word.data(), n, r.offsets.data()));
                        r.hits.resize(n);
                        for (size_t k = 0; k < n; ++k) {
                                r.hits[k].payload = word[k];
                                r.hits[k].pos = pos[k];
                                r.hits[k].payloadLen = len[k];
                        }
                        return r;
                }

                // ---- iterator factories == queryexec_ctx::build_iterator's leaves and combinators (exec.cpp:253-449)
                Codecs::PostingsListIterator *term(const std::string &t) {
                        auto dec = new_postings_decoder(t, resolve_term_ctx(t));
                        auto it = dec->new_iterator();
                        registry.emplace_back(it);
                        return it;
                }
                template <class T, class... A>
                T *reg(A &&... a) {
                        auto p = new T(std::forward<A>(a)...);
                        registry.emplace_back(p);
                        return p;
                }
                DocsSetIterators::Iterator *conjunction(std::vector<DocsSetIterators::Iterator *> its) { return reg<DocsSetIterators::Conjuction>(its.data(), uint16_t(its.size())); }
                DocsSetIterators::Iterator *disjunction(std::vector<DocsSetIterators::Iterator *> its) { return reg<DocsSetIterators::Disjunction>(its.data(), uint16_t(its.size())); }
                DocsSetIterators::Iterator *some(std::vector<DocsSetIterators::Iterator *> its, uint16_t minMatch) { return reg<DocsSetIterators::DisjunctionSome>(its.data(), uint16_t(its.size()), minMatch); } // exec.cpp:276-283
                DocsSetIterators::Iterator *optional(DocsSetIterators::Iterator *main, DocsSetIterators::Iterator *opt) { return reg<DocsSetIterators::Optional>(main, opt); } // exec.cpp:366-377
                DocsSetIterators::Iterator *filter(DocsSetIterators::Iterator *req, DocsSetIterators::Iterator *excl) { return reg<DocsSetIterators::Filter>(req, excl); } // exec.cpp:424-427
                DocsSetIterators::Iterator *phrase(const std::vector<std::string> &terms) {
                        std::vector<Codecs::PostingsListIterator *> its;
                        for (const auto &t : terms)
                                its.push_back(term(t));
                        return reg<DocsSetIterators::Phrase>(its.data(), uint16_t(its.size()));
                }
        };

        // ------------------------------------------------------------------ BM25 (similarity.h:165-255)
        namespace Similarity {
                struct IndexSourcesCollectionBM25Scorer : public IndexSourcesCollectionTermsScorer {
                        static constexpr float k1{1.2f};
                        struct Scorer final : public IndexSourceTermsScorer {
                                struct Weight final : public ScorerWeight {
                                        const double idf;
                                        explicit Weight(double i)
                                            : idf{i} {}
                                };
                                using IndexSourceTermsScorer::IndexSourceTermsScorer;
                                // similarity.h:179-181: evaluated in float precision, kept as double
                                static double idf(const uint32_t docFreq, const uint64_t docsCnt) { return std::log(1 + (docsCnt - docFreq + 0.5f) / (docFreq + 0.5f)); }
                                ScorerWeight *new_scorer_weight(const std::string *terms, uint16_t cnt) override {
                                        double w = 0;
                                        for (uint16_t i = 0; i != cnt; ++i)
                                                w += idf(src->resolve_term_ctx(terms[i]).documents, src->default_field_stats().docsCnt);
                                        return new Weight(w);
                                }
                                // similarity.h:228-235 (host copy of what the device evaluates)
                                float score(isrc_docid_t, uint16_t freq, const ScorerWeight *w) override {
                                        return float(static_cast<const Weight *>(w)->idf * float(freq) / double(freq + k1));
                                }
                                int device_similarity() const override { return TRI_SIM_BM25; }
                                double device_weight(const ScorerWeight *w) const override { return static_cast<const Weight *>(w)->idf; }
                        };
                        IndexSourceTermsScorer *new_source_scorer(IndexSource *s) override { return new Scorer(this, s); }
                };

                // similarity.h:75-163: idf = log((docsCnt + 1) / double(df + 1)) + 1, tf = sqrt(float freq), score = tf * weight
                struct IndexSourcesCollectionTFIDFScorer : public IndexSourcesCollectionTermsScorer {
                        struct Scorer final : public IndexSourceTermsScorer {
                                struct Weight final : public ScorerWeight {
                                        const double v;
                                        explicit Weight(double value)
                                            : v{value} {}
                                };
                                using IndexSourceTermsScorer::IndexSourceTermsScorer;
                                static double idf(const uint32_t docFreq, const uint64_t docsCnt) { return std::log((docsCnt + 1) / double(docFreq + 1)) + 1.0; }
                                ScorerWeight *new_scorer_weight(const std::string *terms, uint16_t cnt) override {
                                        double w = 0;
                                        for (uint16_t i = 0; i != cnt; ++i)
                                                w += idf(src->resolve_term_ctx(terms[i]).documents, src->default_field_stats().docsCnt);
                                        return new Weight(w);
                                }
                                float score(isrc_docid_t, uint16_t freq, const ScorerWeight *w) override { return std::sqrt(float(freq)) * static_cast<const Weight *>(w)->v; }
                                int device_similarity() const override { return TRI_SIM_TFIDF; }
                                double device_weight(const ScorerWeight *w) const override { return static_cast<const Weight *>(w)->v; }
                        };
                        IndexSourceTermsScorer *new_source_scorer(IndexSource *s) override { return new Scorer(this, s); }
                };

                // similarity.h:56-72: score = freq, no weight
                struct IndexSourcesCollectionTrivialScorer : public IndexSourcesCollectionTermsScorer {
                        struct Scorer final : public IndexSourceTermsScorer {
                                using IndexSourceTermsScorer::IndexSourceTermsScorer;
                                ScorerWeight *new_scorer_weight(const std::string *, uint16_t) override { return nullptr; }
                                float score(isrc_docid_t, uint16_t freq, const ScorerWeight *) override { return freq; }
                                int device_similarity() const override { return TRI_SIM_TRIVIAL; }
                                double device_weight(const ScorerWeight *) const override { return 0.0; }
                        };
                        IndexSourceTermsScorer *new_source_scorer(IndexSource *s) override { return new Scorer(this, s); }
                };
        } // namespace Similarity

        // An IndexDocumentsFilter the DEVICE applies (include/trinity_hip.h, per-query document filters): built once from a docID list — the documents to drop, or
        // with keep = true the only documents a query may match — or from a predicate evaluated once over the source's documents 1 .. docsCnt
        // (matches.h:199: true = disregard the document).  It belongs to its source and goes before it.  filter() answers from the same set, for a caller
        // that still asks on the host.
        class DeviceDocumentsFilter final : public IndexDocumentsFilter {
                tri_filter *h{nullptr};
                std::vector<docid_t> ids; // ascending, distinct
                bool keep{false};

                void upload(IndexSource *src) {
                        std::sort(ids.begin(), ids.end());
                        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
                        check(tri_filter_create(src->handle(), ids.data(), ids.size(), keep ? TRI_FILTER_KEEP : TRI_FILTER_DROP, &h));
                }

              public:
                DeviceDocumentsFilter(IndexSource *src, std::vector<docid_t> docids, const bool keepOnly = false)
                    : ids(std::move(docids)), keep{keepOnly} {
                        upload(src);
                }
                template <class Pred, class = decltype(bool(std::declval<Pred &>()(docid_t{})))>
                DeviceDocumentsFilter(IndexSource *src, Pred &&disregard) {
                        const uint32_t n = src->default_field_stats().docsCnt;
                        for (docid_t d = 1; d <= n; ++d)
                                if (disregard(d))
                                        ids.push_back(d);
                        upload(src);
                }
                ~DeviceDocumentsFilter() override { tri_filter_destroy(h); }
                DeviceDocumentsFilter(const DeviceDocumentsFilter &) = delete;
                bool filter(const docid_t id) override { return std::binary_search(ids.begin(), ids.end(), id) != keep; }
                tri_filter *device_filter() override { return h; }
        };

        // ---- facet counts: "just count or collect documents matching a query" (exec.h:12-23), by a per-document attribute.  A DeviceColumn holds the attribute of
        // every docID of ONE source, on the host (the replay path reads it) and on the device (tri_column_create); closed before its source.
        class DeviceColumn final {
                tri_column *h{nullptr};
                IndexSource *const src;
                std::vector<uint32_t> vals; // [docsCnt + 1]: vals[d] for docID d

              public:
                DeviceColumn(IndexSource *s, std::vector<uint32_t> values) : src{s}, vals(std::move(values)) { check(tri_column_create(src->handle(), vals.data(), vals.size(), &h)); }
                template <class Fn, class = decltype(uint32_t(std::declval<Fn &>()(docid_t{})))>
                DeviceColumn(IndexSource *s, Fn &&attribute) : src{s} { // attribute(docID) for 1 .. docsCnt
                        const uint32_t n = src->default_field_stats().docsCnt;
                        vals.assign(size_t(n) + 1, 0);
                        for (docid_t d = 1; d <= n; ++d)
                                vals[d] = attribute(d);
                        check(tri_column_create(src->handle(), vals.data(), vals.size(), &h));
                }
                ~DeviceColumn() { tri_column_destroy(h); }
                DeviceColumn(const DeviceColumn &) = delete;
                tri_column *handle() const { return h; }
                IndexSource *source() const { return src; }
                const std::vector<uint32_t> &values() const { return vals; }
        };

        // An IndexDocumentsFilter whose rule reads the documents' ATTRIBUTES: a predicate — 1 .. TRI_PRED_MAX_CLAUSES RANGE / SET clauses over DeviceColumns of one source,
        // all of them or (any) at least one — evaluated on the device over the resident columns (tri_filters_from_columns: no docID list crosses PCIe).  keepOnly
        // (the default): the documents the predicate holds for are the only ones a query may match; else they are disregarded.  `also`: a device filter of the same
        // source whose disregarded documents this one disregards too.  filter(id) answers from the columns' host copies through column_pred.hpp — the same rule, for
        // a caller that asks on the host and for the replay: with onDevice == false device_filter() is nullptr and exec_query asks filter() per replayed document.
        // It belongs to its source and goes before it.  Like the tri_filter it wraps it does not reference its columns once it is built: the constructor copies the
        // host values of the distinct columns its clauses name, so filter() and the replay stay valid after the DeviceColumns are gone.
        class ColumnPredicateFilter final : public IndexDocumentsFilter {
              public:
                struct Clause {
                        const DeviceColumn *column;
                        uint32_t kind{TRI_CLAUSE_RANGE};
                        bool negate{false};
                        uint32_t lo{0}, hi{0};     // RANGE: lo <= value <= hi, unsigned
                        std::vector<uint32_t> set; // SET: each below TRI_FACET_MAX_BUCKETS
                        static Clause range(const DeviceColumn *c, const uint32_t lo, const uint32_t hi, const bool negate = false) { return Clause{c, TRI_CLAUSE_RANGE, negate, lo, hi, {}}; }
                        static Clause among(const DeviceColumn *c, std::vector<uint32_t> values, const bool negate = false) { return Clause{c, TRI_CLAUSE_SET, negate, 0, 0, std::move(values)}; }
                };

              private:
                tri_filter *h{nullptr};
                std::vector<Clause> clauses;
                std::vector<tri_clause> raw;
                std::vector<std::pair<const tri_column *, std::vector<uint32_t>>> hostValues; // the distinct columns' values, copied: by handle
                tri_predicate pred{};
                IndexDocumentsFilter *const alsoHost;
                const int mode;
                const bool device;

              public:
                ColumnPredicateFilter(IndexSource *src, std::vector<Clause> cl, const bool any = false, const bool keepOnly = true, IndexDocumentsFilter *also = nullptr, const bool onDevice = true)
                    : clauses(std::move(cl)), alsoHost{also}, mode{keepOnly ? TRI_FILTER_KEEP : TRI_FILTER_DROP}, device{onDevice} {
                        for (const Clause &c : clauses) {
                                if (!c.column || c.column->source() != src)
                                        throw invalid_argument("ColumnPredicateFilter: a clause's column belongs to another source");
                                raw.push_back(tri_clause{c.column->handle(), c.kind, c.negate ? 1u : 0u, c.lo, c.hi, c.set.empty() ? nullptr : c.set.data(), uint32_t(c.set.size()), 0});
                                if (std::none_of(hostValues.begin(), hostValues.end(), [&](const auto &hv) { return hv.first == c.column->handle(); }))
                                        hostValues.emplace_back(c.column->handle(), c.column->values());
                        }
                        for (Clause &c : clauses)
                                c.column = nullptr; // (not kept: the columns may go before the filter)
                        if (also && !also->device_filter())
                                throw invalid_argument("ColumnPredicateFilter: the `also` filter has no device bitmap");
                        pred = tri_predicate{raw.data(), uint32_t(raw.size()), any ? 1u : 0u, also ? also->device_filter() : nullptr, 0};
                        check(tri_filters_from_columns(src->handle(), &pred, 1, mode, &h));
                }
                ~ColumnPredicateFilter() override { tri_filter_destroy(h); }
                ColumnPredicateFilter(const ColumnPredicateFilter &) = delete;
                bool filter(const docid_t id) override {
                        const bool also = alsoHost && alsoHost->filter(id);
                        return colpred::drops(pred, id, mode, also, [this](const tri_column *c) {
                                for (const auto &hv : hostValues)
                                        if (hv.first == c)
                                                return hv.second.data();
                                return static_cast<const uint32_t *>(nullptr); // (unreachable: the predicate names the copied columns alone)
                        });
                }
                tri_filter *device_filter() override { return device ? h : nullptr; }
                // the bitmap the device applies (tri_filter_bitmap): bit id & 31 of word id >> 5 set = document id is disregarded
                std::vector<uint32_t> bitmap() const {
                        size_t n = 0;
                        uint32_t none = 0;
                        tri_filter_bitmap(h, &none, 0, &n); // (refused for its capacity: leaves the extent)
                        std::vector<uint32_t> words(n);
                        check(tri_filter_bitmap(h, words.data(), words.size(), &n));
                        return words;
                }
        };

        // The application's consider(id) / consider(ids, cnt) when it counts the matches by attributes — row k has facets[k].nbuckets + 1 counters, and for every
        // considered document counter min(value, nbuckets) goes up by one (the last one is the overflow bucket; facet_rows.hpp) — and the device form of the same:
        // a DocumentsOnly exec_query recognises the counter (device_consumer()) and, with device == true, sets the facets on its batch and reads the rows back
        // (tri_batch_facets) instead of delivering the docID set; device = false keeps the replay through consider(), for comparison.  A facet lists one column per
        // source the counter may run against (a collection: one per source); exec_query binds the counter to its source first.
        struct FacetCounter : public MatchedIndexDocumentsFilter, public DeviceConsumer {
                struct Facet {
                        std::vector<const DeviceColumn *> columns; // one per source
                        uint32_t nbuckets;
                };
                std::vector<Facet> facets;
                bool device{true};
                std::vector<std::vector<uint32_t>> rows; // [facet][nbuckets + 1]
                std::vector<const DeviceColumn *> bound;   // per facet: the column of the source the counter runs against

                explicit FacetCounter(std::vector<Facet> f, const bool onDevice = true) : facets(std::move(f)), device{onDevice} {
                        if (facets.empty() || facets.size() > TRI_FACETS_MAX)
                                throw invalid_argument("FacetCounter: 1 .. TRI_FACETS_MAX facets");
                        for (const auto &x : facets) {
                                if (x.nbuckets < 1 || x.nbuckets > TRI_FACET_MAX_BUCKETS)
                                        throw invalid_argument("FacetCounter: nbuckets 1 .. TRI_FACET_MAX_BUCKETS");
                                rows.emplace_back(size_t(x.nbuckets) + 1, 0u);
                        }
                }
                DeviceConsumer *device_consumer() override { return this; }
                bool on_device() const override { return device; }
                void bind(IndexSource *src) override {
                        bound.assign(facets.size(), nullptr);
                        for (size_t k = 0; k < facets.size(); ++k) {
                                for (const DeviceColumn *c : facets[k].columns)
                                        if (c && c->source() == src)
                                                bound[k] = c;
                                if (!bound[k])
                                        throw invalid_argument("FacetCounter: a facet has no column of the source the query runs against");
                        }
                }
                void consider(const docid_t id) override { consider(&id, 1); }
                void consider(const docid_t *ids, const size_t cnt) override {
                        if (bound.size() != facets.size())
                                throw invalid_argument("FacetCounter: not bound to a source (exec_query binds it)");
                        for (size_t k = 0; k < facets.size(); ++k)
                                facet_rows::count(rows[k].data(), bound[k]->values().data(), bound[k]->values().size(), facets[k].nbuckets, ids, cnt);
                }
                // the device form: the specs for tri_batch_set_facets ...
                std::vector<tri_facet> specs() const {
                        std::vector<tri_facet> out;
                        for (size_t k = 0; k < facets.size(); ++k)
                                out.push_back(tri_facet{bound[k]->handle(), facets[k].nbuckets, 0});
                        return out;
                }
                void install(tri_batch *b) override { const auto s = specs(); check(tri_batch_set_facets(b, s.data(), s.size())); }
                // ... and the rows of the batch's query q added to the counter's
                void read(tri_batch *b, const size_t q, const size_t nq) override {
                        std::vector<uint32_t> all;
                        for (size_t k = 0; k < facets.size(); ++k) {
                                const size_t w = size_t(facets[k].nbuckets) + 1;
                                all.resize(nq * w);
                                check(tri_batch_facets(b, k, all.data(), all.size()));
                                for (size_t i = 0; i < w; ++i)
                                        rows[k][i] += all[q * w + i];
                        }
                }
                // The counters of a collection's sources (exec_query's collection form, one FacetCounter per source) summed, widened: the host form of tri_cbatch_facets.
                static std::vector<uint64_t> sum(const std::vector<std::unique_ptr<FacetCounter>> &parts, const size_t k) {
                        std::vector<uint64_t> out;
                        for (const auto &p : parts) {
                                if (k >= p->rows.size() || (!out.empty() && out.size() != p->rows[k].size()))
                                        throw invalid_argument("FacetCounter::sum: the parts disagree in their facets");
                                out.resize(p->rows[k].size(), 0);
                                facet_rows::add(out.data(), p->rows[k].data(), out.size());
                        }
                        return out;
                }
        };

        // The application's consider(id) / consider(ids, cnt) when it lists the first K matches by an attribute — (value ascending, docID ascending), or descending:
        // (value descending, docID ascending); order_rows.hpp — and the device form of the same: a DocumentsOnly exec_query recognises the filter (device_consumer())
        // and, with device == true, sets the order on its batch and reads the row back (tri_batch_ordered) instead of delivering the docID set; device = false keeps
        // the replay through consider(), for comparison.  columns: one per source the filter may run against (a collection: one per source); exec_query binds it first.
        struct ColumnOrder : public MatchedIndexDocumentsFilter, public DeviceConsumer {
                std::vector<const DeviceColumn *> columns; // one per source
                uint32_t topk;
                bool descending, device;
                const DeviceColumn *bound{nullptr};
                std::vector<uint64_t> keys; // the first topk so far, ascending (order_rows::key)

                ColumnOrder(std::vector<const DeviceColumn *> cols, const uint32_t k, const bool desc = false, const bool onDevice = true)
                    : columns(std::move(cols)), topk{k}, descending{desc}, device{onDevice} {
                        if (topk < 1 || topk > TRI_ORDER_MAX_TOPK)
                                throw invalid_argument("ColumnOrder: topk 1 .. TRI_ORDER_MAX_TOPK");
                }
                DeviceConsumer *device_consumer() override { return this; }
                bool on_device() const override { return device; }
                void bind(IndexSource *src) override {
                        bound = nullptr;
                        for (const DeviceColumn *c : columns)
                                if (c && c->source() == src)
                                        bound = c;
                        if (!bound)
                                throw invalid_argument("ColumnOrder: no column of the source the query runs against");
                }
                void consider(const docid_t id) override { consider(&id, 1); }
                void consider(const docid_t *ids, const size_t cnt) override {
                        if (!bound)
                                throw invalid_argument("ColumnOrder: not bound to a source (exec_query binds it)");
                        order_rows::offer(keys, bound->values().data(), bound->values().size(), topk, descending, ids, cnt);
                }
                // the device form: the spec for tri_batch_set_order ...
                tri_order spec() const { return tri_order{bound->handle(), topk, descending ? 1u : 0u, 0u}; }
                void install(tri_batch *b) override { const tri_order s = spec(); check(tri_batch_set_order(b, &s)); }
                // ... and the row of the batch's query q merged into the list
                void read(tri_batch *b, const size_t q, const size_t nq) override {
                        std::vector<uint32_t> d(nq * topk), v(nq * topk), c(nq);
                        check(tri_batch_ordered(b, d.data(), v.data(), c.data()));
                        std::vector<uint64_t> row;
                        for (uint32_t i = 0; i < c[q]; ++i)
                                row.push_back(uint64_t(descending ? ~v[q * topk + i] : v[q * topk + i]) << 32 | d[q * topk + i]);
                        keys = order_rows::blend({keys, row}, topk);
                }
                std::vector<std::pair<docid_t, uint32_t>> list() const { // (docID, value), best first
                        std::vector<std::pair<docid_t, uint32_t>> out;
                        for (const uint64_t x : keys)
                                out.emplace_back(order_rows::docid_of(x), order_rows::value_of(x, descending));
                        return out;
                }
                // The lists of a collection's sources (exec_query's collection form, one ColumnOrder per source, oldest first) blended into one by (value, docID,
                // source): a docID of several sources is listed once per source.  The host form of tri_cbatch_ordered.
                static std::vector<std::pair<docid_t, uint32_t>> blend(const std::vector<std::unique_ptr<ColumnOrder>> &parts) {
                        std::vector<std::vector<uint64_t>> lists;
                        for (const auto &p : parts) {
                                if (p->topk != parts[0]->topk || p->descending != parts[0]->descending)
                                        throw invalid_argument("ColumnOrder::blend: the parts disagree in topk or direction");
                                lists.push_back(p->keys);
                        }
                        std::vector<std::pair<docid_t, uint32_t>> out;
                        if (!parts.empty())
                                for (const uint64_t x : order_rows::blend(lists, parts[0]->topk))
                                        out.emplace_back(order_rows::docid_of(x), order_rows::value_of(x, parts[0]->descending));
                        return out;
                }
        };

        // The application's consider(id) / consider(ids, cnt) when it adds up an attribute of the matches — the price range, the average rating per category, revenue
        // per brand: row k has stats[k].nbuckets + 1 records (one without a group column), and the record of bucket min(group, nbuckets) takes every considered
        // document's value: count, sum, min, max (stats_rows.hpp) — and the device form of the same: a DocumentsOnly exec_query recognises the counter
        // (device_consumer()) and, with device == true, sets the stats on its batch and reads the rows back (tri_batch_stats) instead of delivering the docID set;
        // device = false keeps the replay through consider(), for comparison.  A stat lists one column per source the counter may run against (a collection: one
        // per source); exec_query binds the counter to its source first.
        struct StatsCounter : public MatchedIndexDocumentsFilter, public DeviceConsumer {
                struct Stat {
                        std::vector<const DeviceColumn *> groups; // one per source; empty: ungrouped, one bucket (nbuckets 0)
                        uint32_t nbuckets;
                        std::vector<const DeviceColumn *> values; // one per source
                };
                std::vector<Stat> stats;
                bool device{true};
                std::vector<std::vector<stats_rows::Record>> rows; // [stat][nbuckets + 1]
                std::vector<const DeviceColumn *> bound_group, bound_value; // per stat: the columns of the source the counter runs against (group: nullptr when ungrouped)

                explicit StatsCounter(std::vector<Stat> st, const bool onDevice = true) : stats(std::move(st)), device{onDevice} {
                        if (stats.empty() || stats.size() > TRI_STATS_MAX)
                                throw invalid_argument("StatsCounter: 1 .. TRI_STATS_MAX stats");
                        for (const auto &x : stats) {
                                if (x.groups.empty() ? x.nbuckets != 0 : (x.nbuckets < 1 || x.nbuckets > TRI_FACET_MAX_BUCKETS))
                                        throw invalid_argument("StatsCounter: nbuckets 1 .. TRI_FACET_MAX_BUCKETS with a group column, 0 without");
                                rows.emplace_back(size_t(x.nbuckets) + 1);
                        }
                }
                DeviceConsumer *device_consumer() override { return this; }
                bool on_device() const override { return device; }
                void bind(IndexSource *src) override {
                        const auto of = [src](const std::vector<const DeviceColumn *> &cols) {
                                const DeviceColumn *out = nullptr;
                                for (const DeviceColumn *c : cols)
                                        if (c && c->source() == src)
                                                out = c;
                                return out;
                        };
                        bound_group.assign(stats.size(), nullptr);
                        bound_value.assign(stats.size(), nullptr);
                        for (size_t k = 0; k < stats.size(); ++k) {
                                bound_group[k] = of(stats[k].groups);
                                bound_value[k] = of(stats[k].values);
                                if (!bound_value[k] || (!stats[k].groups.empty() && !bound_group[k]))
                                        throw invalid_argument("StatsCounter: a stat has no column of the source the query runs against");
                        }
                }
                void consider(const docid_t id) override { consider(&id, 1); }
                void consider(const docid_t *ids, const size_t cnt) override {
                        if (bound_value.size() != stats.size())
                                throw invalid_argument("StatsCounter: not bound to a source (exec_query binds it)");
                        for (size_t k = 0; k < stats.size(); ++k)
                                stats_rows::count(rows[k].data(), bound_group[k] ? bound_group[k]->values().data() : nullptr, bound_value[k]->values().data(), bound_value[k]->values().size(),
                                                  stats[k].nbuckets, ids, cnt);
                }
                // the device form: the specs for tri_batch_set_stats ...
                std::vector<tri_stat> specs() const {
                        std::vector<tri_stat> out;
                        for (size_t k = 0; k < stats.size(); ++k)
                                out.push_back(tri_stat{bound_group[k] ? bound_group[k]->handle() : nullptr, bound_value[k]->handle(), stats[k].nbuckets, 0});
                        return out;
                }
                void install(tri_batch *b) override { const auto s = specs(); check(tri_batch_set_stats(b, s.data(), s.size())); }
                // ... and the rows of the batch's query q combined into the counter's
                void read(tri_batch *b, const size_t q, const size_t nq) override {
                        for (size_t k = 0; k < stats.size(); ++k) {
                                const size_t w = size_t(stats[k].nbuckets) + 1;
                                std::vector<uint64_t> sums(nq * w);
                                std::vector<uint32_t> counts(nq * w), mins(nq * w), maxs(nq * w);
                                check(tri_batch_stats(b, k, sums.data(), counts.data(), mins.data(), maxs.data(), nq * w));
                                if (stats_rows::add(rows[k].data(), sums.data() + q * w, counts.data() + q * w, mins.data() + q * w, maxs.data() + q * w, w) != w)
                                        throw invalid_argument("StatsCounter: a sum wraps 64 bits");
                        }
                }
                // The records of a collection's sources (exec_query's collection form, one StatsCounter per source) combined: the host form of tri_cbatch_stats.
                static std::vector<stats_rows::Record> combine(const std::vector<std::unique_ptr<StatsCounter>> &parts, const size_t k) {
                        std::vector<stats_rows::Record> out;
                        for (const auto &p : parts) {
                                if (k >= p->rows.size() || (!out.empty() && out.size() != p->rows[k].size()))
                                        throw invalid_argument("StatsCounter::combine: the parts disagree in their stats");
                                out.resize(p->rows[k].size());
                                if (stats_rows::add(out.data(), p->rows[k].data(), out.size()) != out.size())
                                        throw invalid_argument("StatsCounter::combine: a sum wraps 64 bits");
                        }
                        return out;
                }
        };

        // ------------------------------------------------------------------ execution
        struct BatchDeleter {
                void operator()(tri_batch *b) const { tri_batch_destroy(b); }
        };
        using BatchPtr = std::unique_ptr<tri_batch, BatchDeleter>;

        inline void validate_flags(const uint32_t f) { // exec.h:45-48
                const auto mask = f & (unsigned(ExecFlags::DocumentsOnly) | unsigned(ExecFlags::AccumulatedScoreScheme));
                if (mask && (mask & (mask - 1)))
                        throw invalid_argument("DocumentsOnly and AccumulatedScoreScheme are mutually exclusive modes");
        }

        // Lower iterator trees (the mirror of build_iterator's output), attach one ScorerWeight per TERM token
        // (docset_iterators_scorers.cpp:16-22), create + run one batch.
        // docFilters: per query its device filter (IndexDocumentsFilter::device_filter; nullptr: none), installed before the run; empty: no query has one.
        inline BatchPtr run_batch(IndexSource *src, const std::vector<DocsSetIterators::Iterator *> &roots, uint32_t flags, uint32_t topk,
                                  Similarity::IndexSourceTermsScorer *scorer, const std::vector<tri_filter *> &docFilters = {},
                                  const std::function<void(tri_batch *, const std::vector<uint32_t> &, const std::vector<tri_query> &)> &beforeRun = nullptr) {
                validate_flags(flags);
                const bool scored = flags & unsigned(ExecFlags::AccumulatedScoreScheme);
                if (!(flags & (unsigned(ExecFlags::DocumentsOnly) | unsigned(ExecFlags::AccumulatedScoreScheme))))
                        flags = TRI_FLAG_MATCHED_TERMS; // no ExecFlags: exec_query's default mode (exec.cpp:1350-1501)
                if (scored && !scorer)
                        throw invalid_argument("IndexSourceTermsScorer not set"); // exec.h:105-108
                std::vector<uint32_t> prog;
                std::vector<double> weights;
                std::vector<tri_query> qs;
                for (auto r : roots) {
                        const uint32_t off = uint32_t(prog.size());
                        r->lower(prog, weights, scored ? scorer : nullptr);
                        qs.push_back({off, uint32_t(prog.size()) - off});
                }
                tri_batch *b = nullptr;
                check(tri_batch_create(src->handle(), prog.data(), prog.size(), qs.data(), qs.size(), scored ? weights.data() : nullptr, flags, topk,
                                       scored ? scorer->device_similarity() : TRI_SIM_BM25, &b));
                BatchPtr bp(b);
                // (a shape the planner does not lower is left out of the batch with a status, not refused as a whole: these entry points
                //  run one caller query at a time — exec_queries: one caller batch —, so such a query surfaces as the exception it always did)
                std::vector<int32_t> st(qs.size(), TRI_OK);
                check(tri_batch_query_status(b, st.data()));
                for (const int32_t x : st)
                        if (x != TRI_OK)
                                check(x);
                if (!docFilters.empty()) {
                        if (docFilters.size() != qs.size())
                                throw invalid_argument("one document filter per query");
                        std::vector<tri_filter *> distinct;
                        std::vector<uint32_t> of_query(qs.size(), 0xffffffffu);
                        for (size_t q = 0; q < qs.size(); ++q)
                                if (docFilters[q]) {
                                        const auto it = std::find(distinct.begin(), distinct.end(), docFilters[q]);
                                        of_query[q] = uint32_t(it - distinct.begin());
                                        if (it == distinct.end())
                                                distinct.push_back(docFilters[q]);
                                }
                        if (!distinct.empty())
                                check(tri_batch_set_filters(b, distinct.data(), distinct.size(), of_query.data()));
                }
                if (beforeRun) // (the default mode's device ranker: set on the compiled batch, from the program it was compiled from)
                        beforeRun(b, prog, qs);
                check(tri_batch_run(b));
                check(tri_batch_sync(b));
                return bp;
        }

        class DocsSetSpan { // docset_spans.h:36-90
              public:
                virtual isrc_docid_t process(MatchesProxy *, const isrc_docid_t min, const isrc_docid_t max) = 0;
                virtual uint64_t cost() = 0;
                virtual ~DocsSetSpan() = default;
        };

        // The batch-granular seam: the FIRST process() runs the whole iterator tree on the GPU — one tri_batch_create / run / read-back —, and the span
        // keeps the ascending match list (+ scores); every process(mp, min, max) then replays the matches of [min, max) from it, found by a
        // binary search, through the caller's MatchesProxy in ascending docID order, as GenericDocsSetSpan::process (docset_spans.cpp:269-290)
        // and the window-union spans (98-173, 681-790) do, and returns the first match >= max.  A composite caller that walks the docID space
        // window by window (docset_spans.h:292-296: min == max with no proxy means "just advance") therefore costs ONE device batch for the
        // whole walk, not one per window (round 4 compiled and ran the query again on every call); batches_run() says how many there were.
        class GpuDocsSetSpan final : public DocsSetSpan {
                DocsSetIterators::Iterator *const root;
                const uint32_t flags;
                Similarity::IndexSourceTermsScorer *const scorer;
                tri_filter *const docFilter; // the application's filter, applied by the device (nullptr: none, or one the caller applies while it replays)
                std::vector<uint32_t> ids; // the query's matches, ascending (filled by the first process())
                std::vector<double> sc;    // ... and their scores (AccumulatedScoreScheme)
                bool ran{false};
                unsigned batches{0};

                void run_once() {
                        if (ran)
                                return;
                        const bool scored = flags & unsigned(ExecFlags::AccumulatedScoreScheme);
                        auto b = run_batch(root->isrc, {root}, flags, 0, scorer, docFilter ? std::vector<tri_filter *>{docFilter} : std::vector<tri_filter *>{});
                        ++batches;
                        size_t n = 0;
                        check(tri_batch_docset(b.get(), 0, nullptr, 0, &n));
                        ids.resize(n);
                        sc.resize(scored ? n : 0);
                        if (n) {
                                check(tri_batch_docset(b.get(), 0, ids.data(), n, &n));
                                if (scored)
                                        check(tri_batch_scores(b.get(), 0, sc.data(), n, &n));
                        }
                        ran = true;
                }

              public:
                GpuDocsSetSpan(DocsSetIterators::Iterator *r, uint32_t f, Similarity::IndexSourceTermsScorer *s, tri_filter *df = nullptr)
                    : root{r}, flags{f}, scorer{s}, docFilter{df} {}
                uint64_t cost() override { return root->cost(); }
                unsigned batches_run() const { return batches; } // device batches this span has compiled and run (1 after any number of windows)
                isrc_docid_t process(MatchesProxy *mp, const isrc_docid_t min, const isrc_docid_t max) override {
                        run_once();
                        const bool scored = !sc.empty();
                        size_t i = size_t(std::lower_bound(ids.begin(), ids.end(), uint32_t(min)) - ids.begin());
                        relevant_document rel;
                        for (; i < ids.size() && ids[i] < max; ++i)
                                if (mp) {
                                        rel.set_document(ids[i]);
                                        rel.score_ = scored ? sc[i] : 0.0;
                                        mp->process(&rel);
                                }
                        return i < ids.size() ? isrc_docid_t(ids[i]) : DocIDsEND;
                }
        };

        // exec.cpp:509-1517 for the two lowered modes: build the span over the iterator tree, process(1, DocIDsEND),
        // deliver through the no-mask handlers (exec.cpp:1213-1229 docs-only, 1322-1341 accumulated score), honouring an
        // IndexDocumentsFilter (matches.h:198-201) and cooperative cancellation (exec.cpp:1505-1510).
        // The default mode: every match is delivered as a matched_document — the query terms that matched it and their hits
        // (prepare_match, queryexec_ctx.cpp:522-648) — rebuilt here from the engine's packed arrays.
        inline void exec_query_default_mode(DocsSetIterators::Iterator *root, IndexSource *src, MatchedIndexDocumentsFilter *mf, IndexDocumentsFilter *df) {
                tri_filter *const onDevice = df ? df->device_filter() : nullptr;
                // a filter that IS the engine's proximity ranker (and no document filter the device does not hold): the ranking is computed on the device, K pairs
                // come back, no match is replayed
                tri_ranker spec{};
                std::vector<double> termWeights;
                std::vector<std::pair<docid_t, double>> *const rankedInto = (!df || onDevice) ? mf->device_ranker(&spec, &termWeights) : nullptr;
                if (rankedInto) {
                        auto b = run_batch(src, {root}, 0, 0, nullptr, onDevice ? std::vector<tri_filter *>{onDevice} : std::vector<tri_filter *>{},
                                           [&](tri_batch *bt, const std::vector<uint32_t> &prog, const std::vector<tri_query> &qs) {
                                                   // the ABI takes a weight per program token: every TERM token gets the weight of its term's place among the query's terms
                                                   uint32_t terms[64], nt = 0;
                                                   check(tri_batch_query_terms_wide(bt, 0, terms, &nt));
                                                   std::vector<double> w(prog.size(), 1.0);
                                                   for (uint32_t i = qs[0].prog_off; i < qs[0].prog_off + qs[0].prog_len; ++i)
                                                           if ((prog[i] >> 28) == TRI_OP_TERM) {
                                                                   const uint32_t k = uint32_t(std::find(terms, terms + nt, prog[i] & 0x0fffffffu) - terms);
                                                                   if (k < nt && k < termWeights.size())
                                                                           w[i] = termWeights[k];
                                                           }
                                                   check(tri_batch_set_ranker(bt, &spec, w.data()));
                                           });
                        std::vector<uint32_t> ids(spec.topk);
                        std::vector<double> scores(spec.topk);
                        uint32_t cnt = 0;
                        check(tri_batch_ranked(b.get(), ids.data(), scores.data(), &cnt));
                        rankedInto->clear();
                        for (uint32_t i = 0; i < cnt; ++i)
                                rankedInto->emplace_back(ids[i], scores[i]);
                        return;
                }
                auto b = run_batch(src, {root}, 0, 0, nullptr, onDevice ? std::vector<tri_filter *>{onDevice} : std::vector<tri_filter *>{});
                if (onDevice)
                        df = nullptr; // (the batch has dropped its documents: nothing to ask per match)
                size_t n = 0, npos = 0;
                check(tri_batch_docset(b.get(), 0, nullptr, 0, &n));
                std::vector<docid_t> ids(n);
                if (n)
                        check(tri_batch_docset(b.get(), 0, ids.data(), n, &n));
                // (the _wide calls: 64-bit masks — a query of up to 64 reportable terms once the caller has set option rich_max_terms on the device; they serve
                //  every query, a narrow one's mask zero-extended)
                uint32_t terms[64], nt = 0;
                check(tri_batch_query_terms_wide(b.get(), 0, terms, &nt));
                check(tri_batch_matched_terms_wide(b.get(), 0, nullptr, nullptr, nullptr, 0, &npos));
                std::vector<uint64_t> present(n);
                std::vector<uint16_t> freq(n * std::max<uint32_t>(nt, 1)), pos(npos);
                check(tri_batch_matched_terms_wide(b.get(), 0, present.data(), freq.data(), pos.data(), pos.size(), &npos));
                std::vector<query_term_ctx> qctx(nt);
                for (uint32_t k = 0; k < nt; ++k) {
                        qctx[k].term.id = exec_term_id_t(k + 1);
                        qctx[k].term.token = src->term_name(terms[k]);
                }
                std::vector<term_hits> th(nt);
                std::vector<matched_query_term> mts(nt);
                std::vector<std::vector<term_hit>> store(nt);
                size_t at = 0;
                try {
                        for (size_t i = 0; i < n; ++i) {
                                matched_document md;
                                md.id = ids[i];
                                md.matchedTerms = mts.data();
                                for (uint32_t k = 0; k < nt; ++k) {
                                        const uint32_t f = freq[i * nt + k];
                                        if ((present[i] >> k) & 1ull) {
                                                store[k].resize(f);
                                                for (uint32_t h = 0; h < f; ++h)
                                                        store[k][h].pos = pos[at + h];
                                                th[k].freq = tokenpos_t(f);
                                                th[k].all = store[k].data();
                                                mts[md.matchedTermsCnt++] = {&qctx[k], &th[k]};
                                        }
                                        at += f;
                                }
                                if (!(df && df->filter(md.id)))
                                        mf->consider(md);
                        }
                } catch (const aborted_search_exception &) {
                }
        }

        // docidupdates.h:15-119.  The documents of a source that newer sources of the collection have updated or deleted.  The reference packs
        // each source's list into banks with a skiplist (updated_documents, pack_updates / unpack_updates) and hands exec_query a
        // masked_documents_registry over the lists of all the newer sources — a bloom filter in front of one scanner per list, tested
        // document by document right before consider() (exec.cpp:914-975).  Its observable behaviour is set membership, and that is what
        // is mirrored: the registry is the union of its lists, it goes to the device as a docID bitmap (tri_index_set_masked) and the
        // matching kernels test it where exec_query does.
        struct updated_documents final {
                std::vector<docid_t> ids; // ascending (what pack_updates sorts them into)
        };
        struct masked_documents_registry final {
                std::vector<docid_t> ids; // ascending, distinct
                // docidupdates.h:121-142 masked_documents_registry::make(const updated_documents *, n)
                static std::unique_ptr<masked_documents_registry> make(const updated_documents *ud, const std::size_t n) {
                        auto r = std::make_unique<masked_documents_registry>();
                        for (std::size_t i = 0; i < n; ++i)
                                r->ids.insert(r->ids.end(), ud[i].ids.begin(), ud[i].ids.end());
                        std::sort(r->ids.begin(), r->ids.end());
                        r->ids.erase(std::unique(r->ids.begin(), r->ids.end()), r->ids.end());
                        return r;
                }
                bool test(const docid_t id) const { return std::binary_search(ids.begin(), ids.end(), id); }
                bool empty() const noexcept { return ids.empty(); }
        };

        inline void exec_query(DocsSetIterators::Iterator *root, IndexSource *src, MatchedIndexDocumentsFilter *matchesFilter, IndexDocumentsFilter *f = nullptr,
                               const uint32_t flags = 0, Similarity::IndexSourceTermsScorer *scorer = nullptr);

        // exec.h:50: exec_query(query, IndexSource *, masked_documents_registry *, MatchedIndexDocumentsFilter *, IndexDocumentsFilter *, flags,
        // scorer) — the reference's own argument order (the query is the lowered iterator tree here).  The registry becomes the source's
        // masked set for this call (nullptr / empty: none), then the query runs as above.
        inline void exec_query(DocsSetIterators::Iterator *root, IndexSource *src, masked_documents_registry *const maskedDocumentsRegistry,
                               MatchedIndexDocumentsFilter *matchesFilter, IndexDocumentsFilter *const f = nullptr, const uint32_t flags = 0,
                               Similarity::IndexSourceTermsScorer *scorer = nullptr) {
                // (the reference's registry is strictly per call, exec.h:50: whatever set the source carried before is back when the call returns,
                //  also when the application's filter throws)
                struct Restore {
                        IndexSource *src;
                        std::vector<docid_t> before;
                        ~Restore() {
                                try {
                                        src->set_masked_documents(before);
                                } catch (...) {
                                }
                        }
                } restore{src, src->masked_documents()};
                src->set_masked_documents(maskedDocumentsRegistry ? maskedDocumentsRegistry->ids : std::vector<docid_t>{});
                exec_query(root, src, matchesFilter, f, flags, scorer);
        }

        inline void exec_query(DocsSetIterators::Iterator *root, IndexSource *src, MatchedIndexDocumentsFilter *matchesFilter, IndexDocumentsFilter *f,
                               const uint32_t flags, Similarity::IndexSourceTermsScorer *scorer) {
                validate_flags(flags);
                if (!(flags & (unsigned(ExecFlags::DocumentsOnly) | unsigned(ExecFlags::AccumulatedScoreScheme))))
                        return exec_query_default_mode(root, src, matchesFilter, f);
                struct Handler final : public MatchesProxy {
                        MatchedIndexDocumentsFilter *mf;
                        IndexDocumentsFilter *df;
                        bool scored;
                        void process(relevant_document_provider *rdp) override {
                                const auto id = rdp->document();
                                if (df && df->filter(id))
                                        return;
                                if (scored)
                                        mf->consider(id, rdp->score());
                                else
                                        mf->consider(id);
                        }
                } handler;
                // a filter the device holds (DeviceDocumentsFilter) is installed with the batch — tri_batch_set_filters — and asked nothing here; a plain host
                // filter is asked per replayed document
                tri_filter *const onDevice = f ? f->device_filter() : nullptr;
                // a facet counter, a column order or a stats counter runs against this source; on the device when nothing but the device decides which documents
                // count (DocumentsOnly, no host filter)
                if (DeviceConsumer *const dc = matchesFilter ? matchesFilter->device_consumer() : nullptr) {
                        dc->bind(src);
                        if (dc->on_device() && (flags & unsigned(ExecFlags::DocumentsOnly)) && (!f || onDevice)) {
                                auto b = run_batch(src, {root}, flags, 0, nullptr, onDevice ? std::vector<tri_filter *>{onDevice} : std::vector<tri_filter *>{},
                                                   [&](tri_batch *bt, const std::vector<uint32_t> &, const std::vector<tri_query> &) { dc->install(bt); });
                                dc->read(b.get(), 0, 1);
                                return;
                        }
                }
                handler.mf = matchesFilter;
                handler.df = onDevice ? nullptr : f;
                handler.scored = flags & unsigned(ExecFlags::AccumulatedScoreScheme);
                GpuDocsSetSpan span(root, flags, scorer, onDevice);
                try {
                        span.process(&handler, 1, DocIDsEND);
                } catch (const aborted_search_exception &) {
                        // search was aborted by the application's filter
                }
        }

        // index_source.cpp:3-30 IndexSourcesCollection: the sources of an index, oldest first, each with the documents it updates or deletes in the older ones.
        // scanner_registry_for(i) is the registry exec_query runs source i under: the union of the lists of the sources newer than i.  (The reference's commit()
        // collects the lists from the sources; here the caller hands each list over with its source.  The sources are borrowed.)
        class IndexSourcesCollection final {
                std::vector<updated_documents> all; // per source, in the order of sources[]

              public:
                std::vector<IndexSource *> sources;

                void insert(IndexSource *is, updated_documents updates = {}) {
                        std::sort(updates.ids.begin(), updates.ids.end());
                        sources.push_back(is);
                        all.push_back(std::move(updates));
                }
                std::unique_ptr<masked_documents_registry> scanner_registry_for(const std::size_t idx) const {
                        if (idx >= all.size())
                                throw invalid_argument("IndexSourcesCollection::scanner_registry_for: no such source");
                        return masked_documents_registry::make(all.data() + idx + 1, all.size() - idx - 1);
                }
        };

        // exec.h:63-81: the query over every source of the collection in sequence, each under its registry, one T per source — "you are expected to
        // merge/reduce/blend them" (ProximityRanker::blend).  roots: the query lowered against each source (roots[i] from sources[i]'s own iterators: term
        // ids are per source).  Every IndexSource holds its own device handle, so the sources' batches are independent, as the reference's executions are.
        template <typename T, typename... Arg>
        std::vector<std::unique_ptr<T>> exec_query(const std::vector<DocsSetIterators::Iterator *> &roots, IndexSourcesCollection *collection, IndexDocumentsFilter *f, const uint32_t flags,
                                                   const Arg &... args) {
                static_assert(std::is_base_of<MatchedIndexDocumentsFilter, T>::value, "expected a MatchedIndexDocumentsFilter subclass");
                validate_flags(flags);
                const std::size_t n = collection->sources.size();
                if (roots.size() != n)
                        throw invalid_argument("exec_query: one lowered query per source of the collection");
                std::vector<std::unique_ptr<T>> out;
                for (std::size_t i = 0; i < n; ++i) {
                        const auto scanner = collection->scanner_registry_for(i);
                        auto filter = std::make_unique<T>(args...);
                        exec_query(roots[i], collection->sources[i], scanner.get(), filter.get(), f, flags);
                        out.push_back(std::move(filter));
                }
                return out;
        }

        // ---- intersect.h:25-47, intersect.cpp:5-217: which subsets of a query's token groups co-occur in documents, and in how many — the engine behind
        // intersection_alternatives' suggestions, on the device (tri_isect_run).  tokens: per query token the set of its synonymous terms, at most 64 sets; a
        // term the source does not know is an unknown token (intersect.cpp:38-43).  The registry becomes the source's masked set for the call, as in exec_query.
        // What differs from the reference's code, on purpose: the stop-word rule is the documented one (the lowest or the highest set bit of a document's mask
        // is in stopwordsMask, intersect.h:15-18 — the same as the reference's only for stopwordsMask == 0), ties of the final order are broken by ascending
        // mask, and a request that overflows the engine's tables (options isect_max_masks / isect_max_runs) throws invalid_argument: the caller keeps its own path.
        // intersection_alternatives (intersect.cpp:219-327) needs the query rewriter (queries_rewrite.h) and is not mirrored.
        inline void intersect_impl(const uint64_t stopwordsMask, const std::vector<std::unordered_set<std::string>> &tokens, IndexSource *const src,
                                   masked_documents_registry *const maskedDocumentsRegistry, std::vector<std::pair<uint64_t, uint32_t>> *const out) {
                if (tokens.empty() || tokens.size() > 64 || !out || !src)
                        throw invalid_argument("intersect_impl: 1 .. 64 token sets, a source and an output vector"); // intersect.cpp:18-19
                struct Restore {
                        IndexSource *src;
                        std::vector<docid_t> before;
                        ~Restore() {
                                try {
                                        src->set_masked_documents(before);
                                } catch (...) {
                                }
                        }
                } restore{src, src->masked_documents()};
                src->set_masked_documents(maskedDocumentsRegistry ? maskedDocumentsRegistry->ids : std::vector<docid_t>{});
                std::vector<uint32_t> terms, first{0};
                for (const auto &set : tokens) {
                        for (const auto &token : set) {
                                const uint32_t id = src->term_id(token);
                                terms.push_back(id == 0x0fffffffu ? 0xffffffffu : id); // (term_id's "no such term" -> tri_isect_run's unknown token)
                        }
                        first.push_back((uint32_t)terms.size());
                }
                terms.push_back(0); // (never null)
                const tri_isect_request req{(uint32_t)tokens.size(), 0, stopwordsMask};
                tri_isect *h = nullptr;
                check(tri_isect_run(src->handle(), &req, 1, terms.data(), first.data(), &h));
                struct Free {
                        tri_isect *h;
                        ~Free() { tri_isect_destroy(h); }
                } free_{h};
                size_t n = 0;
                check(tri_isect_results(h, 0, nullptr, nullptr, 0, &n));
                std::vector<uint64_t> masks(n + 1);
                std::vector<uint32_t> counts(n + 1);
                check(tri_isect_results(h, 0, masks.data(), counts.data(), n, &n));
                for (size_t i = 0; i < n; ++i)
                        out->push_back({masks[i], counts[i]}); // intersect.cpp:165-169
        }
        inline std::vector<std::pair<uint64_t, uint32_t>> intersect(const uint64_t stopwordsMask, const std::vector<std::unordered_set<std::string>> &tokens, IndexSource *src,
                                                                    masked_documents_registry *reg) { // intersect.h:27-32
                std::vector<std::pair<uint64_t, uint32_t>> res;
                intersect_impl(stopwordsMask, tokens, src, reg, &res);
                return res;
        }
        // intersect.cpp:172-201: one run per source under that source's registry (origMask is per source: a token one source does not know is unknown there
        // only), then the lists sorted by mask and equal masks summed
        inline std::vector<std::pair<uint64_t, uint32_t>> intersect(const uint64_t stopwordsMask, const std::vector<std::unordered_set<std::string>> &tokens,
                                                                    IndexSourcesCollection *collection) {
                std::vector<std::pair<uint64_t, uint32_t>> out;
                for (std::size_t i = 0; i != collection->sources.size(); ++i) {
                        const auto scanner = collection->scanner_registry_for(i);
                        intersect_impl(stopwordsMask, tokens, collection->sources[i], scanner.get(), &out);
                }
                std::stable_sort(out.begin(), out.end(), [](const auto &a, const auto &b) noexcept { return a.first < b.first; }); // :184
                std::size_t o = 0;
                for (std::size_t p = 0; p != out.size();) { // :187-197
                        const auto mask = out[p].first;
                        auto cnt = out[p].second;
                        for (++p; p != out.size() && out[p].first == mask; ++p)
                                cnt += out[p].second;
                        out[o++] = {mask, cnt};
                }
                out.resize(o);
                return out;
        }
        // intersect.cpp:203-217: the indices of a mask's set bits, ascending; returns how many
        inline uint8_t intersection_indices(uint64_t mask, uint8_t *const out) {
                uint8_t collected = 0;
                for (; mask; mask &= mask - 1)
                        out[collected++] = (uint8_t)__builtin_ctzll(mask);
                return collected;
        }
        // intersect.h:42-47
        static inline bool sort_intersections(const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) noexcept {
                const auto ca = __builtin_popcountll(a.first), cb = __builtin_popcountll(b.first);
                return cb < ca || (cb == ca && b.second < a.second);
        }

        // The batched sibling of exec_query_par (exec.h:87-177): all queries in ONE engine batch; DocumentsOnly results
        // arrive through consider(ids, cnt) (matches.h:161-165), scored ones through consider(id, score).
        // docFilters: optionally one IndexDocumentsFilter per query (nullptr: none) — filters the device holds (DeviceDocumentsFilter), installed with the batch.
        inline void exec_queries(const std::vector<DocsSetIterators::Iterator *> &roots, IndexSource *src, const std::vector<MatchedIndexDocumentsFilter *> &filters,
                                 const uint32_t flags, Similarity::IndexSourceTermsScorer *scorer = nullptr, const std::vector<IndexDocumentsFilter *> &docFilters = {}) {
                if (roots.size() != filters.size() || (!docFilters.empty() && docFilters.size() != roots.size()))
                        throw invalid_argument("one filter per query");
                std::vector<tri_filter *> onDevice(docFilters.size(), nullptr);
                for (size_t q = 0; q < docFilters.size(); ++q)
                        if (docFilters[q] && !(onDevice[q] = docFilters[q]->device_filter()))
                                throw invalid_argument("exec_queries takes document filters the device holds (DeviceDocumentsFilter)");
                const bool scored = flags & unsigned(ExecFlags::AccumulatedScoreScheme);
                auto b = run_batch(src, roots, flags, 0, scorer, onDevice);
                std::vector<uint32_t> ids;
                std::vector<double> sc;
                if (!scored) {
                        // every set in ONE delivery, each in the form the engine holds it (tri_batch_docsets_mixed): a dense set arrives as the words of a bitmap over
                        // its docID range — a bit per document across PCIe instead of four bytes per match — and is expanded here into consider()'s ids
                        std::vector<uint64_t> offs(roots.size() + 1);
                        std::vector<uint32_t> forms(roots.size() + 1), flat;
                        check(tri_batch_docsets_mixed(b.get(), nullptr, 0, offs.data(), forms.data()));
                        flat.resize(offs.back() + 1);
                        check(tri_batch_docsets_mixed(b.get(), flat.data(), flat.size(), offs.data(), forms.data()));
                        for (size_t q = 0; q < roots.size(); ++q) {
                                const uint32_t *part = flat.data() + offs[q];
                                size_t n = offs[q + 1] - offs[q];
                                if (forms[q]) { // bit j of word i: document 32 i + j
                                        ids.clear();
                                        for (size_t i = 0; i < n; ++i)
                                                for (uint32_t m = part[i]; m; m &= m - 1)
                                                        ids.push_back((uint32_t)(32 * i) + (uint32_t)__builtin_ctz(m));
                                        part = ids.data();
                                        n = ids.size();
                                }
                                try {
                                        filters[q]->consider(part, n);
                                } catch (const aborted_search_exception &) {
                                }
                        }
                        return;
                }
                for (size_t q = 0; q < roots.size(); ++q) {
                        size_t n = 0;
                        check(tri_batch_docset(b.get(), q, nullptr, 0, &n));
                        ids.resize(n);
                        if (n)
                                check(tri_batch_docset(b.get(), q, ids.data(), n, &n));
                        try {
                                if (!scored)
                                        filters[q]->consider(ids.data(), n);
                                else {
                                        sc.resize(n);
                                        if (n)
                                                check(tri_batch_scores(b.get(), q, sc.data(), n, &n));
                                        for (size_t i = 0; i < n; ++i)
                                                filters[q]->consider(ids[i], sc[i]);
                                }
                        } catch (const aborted_search_exception &) {
                        }
                }
        }

        // ------------------------------------------------------------------ out-of-line pieces
        inline uint64_t Codecs::PostingsListIterator::cost() const { return dec->indexTermCtx.documents; }
        inline void Codecs::PostingsListIterator::lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const {
                prog.push_back(TRI_TOK(TRI_OP_TERM, dec->termId));
                double weight = 0;
                if (scorer) {
                        std::unique_ptr<Similarity::ScorerWeight> sw(scorer->new_scorer_weight(&dec->term, 1));
                        weight = scorer->device_weight(sw.get());
                }
                w.push_back(weight);
        }
        inline void DocsSetIterators::Phrase::lower(std::vector<uint32_t> &prog, std::vector<double> &w, Similarity::IndexSourceTermsScorer *scorer) const {
                std::vector<std::string> terms;
                for (auto it : its) {
                        it->lower(prog, w, nullptr);
                        terms.push_back(it->dec->term);
                }
                prog.push_back(TRI_TOK(TRI_OP_PHRASE, its.size()));
                double weight = 0;
                if (scorer) { // similarity.h:209-217: a phrase's weight sums its terms' idf
                        std::unique_ptr<Similarity::ScorerWeight> sw(scorer->new_scorer_weight(terms.data(), uint16_t(terms.size())));
                        weight = scorer->device_weight(sw.get());
                }
                w.push_back(weight);
        }
        // a composite iterator driven by hand materialises its docID set with one DocumentsOnly engine run
        inline void DocsSetIterators::Iterator::materialize() {
                if (materialized)
                        return;
                materialized = true;
                auto b = run_batch(isrc, {this}, unsigned(ExecFlags::DocumentsOnly), 0, nullptr);
                size_t n = 0;
                check(tri_batch_docset(b.get(), 0, nullptr, 0, &n));
                docs.resize(n);
                if (n)
                        check(tri_batch_docset(b.get(), 0, docs.data(), n, &n));
        }
        // a postings list materialises docIDs AND freqs through the codec seam (tri_decode_terms)
        inline void Codecs::PostingsListIterator::materialize() {
                if (materialized)
                        return;
                materialized = true;
                const uint32_t n = dec->indexTermCtx.documents;
                docs.resize(n);
                freqs.resize(n);
                if (!n)
                        return;
                uint64_t offs[2];
                check(tri_decode_terms(isrc->handle(), &dec->termId, 1, docs.data(), freqs.data(), offs));
        }
        inline void Codecs::PostingsListIterator::materialize_hits(DocWordsSpace *dws, term_hit *out) {
                if (!cursor || curDocument.id == DocIDsEND)
                        return; // (no current document)
                if (!hitsFetched) {
                        hitsFetched = true;
                        hitFirst.assign(freqs.size() + 1, 0);
                        for (size_t j = 0; j < freqs.size(); ++j)
                                hitFirst[j + 1] = hitFirst[j] + freqs[j];
                        const size_t n = size_t(hitFirst.back());
                        hitPos.resize(n);
                        hitLen.resize(n);
                        hitPayload.resize(n);
                        uint64_t offs[2];
                        if (n)
                                check(tri_decode_hits(isrc->handle(), &dec->termId, 1, hitPos.data(), hitLen.data(), hitPayload.data(), n, offs));
                }
                const uint64_t at = hitFirst[cursor - 1];
                for (uint32_t h = 0; h < freq; ++h) { // (freq: tokenpos_t, what the caller sized `out` by)
                        out[h].payload = hitPayload[at + h];
                        out[h].pos = hitPos[at + h];
                        out[h].payloadLen = hitLen[at + h];
                        if (dws && out[h].pos)
                                dws->set(dec->execCtxTermID, out[h].pos);
                }
        }

        // ---- the percolator (percolator.h:1-60, percolator.cpp:5-137): documents matched against stored queries.  The text-to-tree step (compile_query)
        //      stays out, as it does for queries: a percolator_query is built from a postfix program whose TERM operands index the query's own distinct terms.
        struct percolator_document_proxy { // percolator.h:10-20
                virtual bool match_term(const uint16_t term) = 0;
                virtual bool match_phrase(const uint16_t *phraseTerms, const uint16_t phraseTermsCnt) = 0;
                virtual ~percolator_document_proxy() = default;
        };

        class percolator_query final { // percolator.h:22-60
              public:
                percolator_query() = default; // constfalse (percolator.cpp:76-78): never matches
                // program: postfix tokens (TRI_TOK), TERM operands = indices into `terms` (the query's distinct terms, as CCTX::resolve_query_term numbers them)
                percolator_query(std::vector<uint32_t> program, std::vector<std::string> terms) : prog(std::move(program)), distinct(std::move(terms)) {}
                const std::string &term_by_index(const uint16_t idx) const { return distinct.at(idx); } // percolator.h:52
                const std::vector<std::string> &distinct_terms() const { return distinct; }
                const std::vector<uint32_t> &program() const { return prog; }
                operator bool() const noexcept { return !prog.empty(); } // percolator.h:56-58
                // percolator.cpp:5-137, the recursion over exec_nodes as a walk over the postfix program: one document, one thread
                bool match(percolator_document_proxy &src) const {
                        struct V {
                                bool v;
                                uint16_t term;
                        };
                        std::vector<V> st;
                        for (const uint32_t t : prog) {
                                const uint32_t op = t >> 28, arg = t & 0x0fffffffu;
                                if (op == TRI_OP_TERM) {
                                        st.push_back({src.match_term(uint16_t(arg)), uint16_t(arg)}); // match_term, :11-12
                                        continue;
                                }
                                const uint32_t n = op == TRI_OP_SOME ? (arg & 0xffffu) : arg;
                                if (n < 1 || n > st.size())
                                        throw invalid_argument("percolator_query: malformed program");
                                const V *k = st.data() + st.size() - n;
                                bool v = false;
                                uint32_t cnt = 0;
                                for (uint32_t i = 0; i < n; ++i)
                                        cnt += k[i].v;
                                switch (op) {
                                        case TRI_OP_AND: // matchallterms / logicaland / matchallnodes
                                                v = cnt == n;
                                                break;
                                        case TRI_OP_OR: // matchanyterms / logicalor / matchanynodes
                                                v = cnt != 0;
                                                break;
                                        case TRI_OP_NOT: // unarynot :45-46, logicalnot :86-90
                                                v = n == 1 ? !k[0].v : (k[0].v && !k[1].v);
                                                break;
                                        case TRI_OP_OPT: // logicaland(x, consttrueexpr), :80-84, :129
                                                v = k[0].v;
                                                break;
                                        case TRI_OP_SOME: // matchsome :98-107
                                                v = cnt >= (arg >> 16);
                                                break;
                                        case TRI_OP_PHRASE: { // match_phrase, :13-17
                                                std::vector<uint16_t> words(n);
                                                for (uint32_t i = 0; i < n; ++i)
                                                        words[i] = k[i].term;
                                                v = n == 1 ? k[0].v : src.match_phrase(words.data(), uint16_t(n));
                                        } break;
                                        default:
                                                throw invalid_argument("percolator_query: malformed program");
                                }
                                st.resize(st.size() - n);
                                st.push_back({v, 0});
                        }
                        return st.size() == 1 && st[0].v;
                }

              private:
                std::vector<uint32_t> prog;
                std::vector<std::string> distinct;
        };

        // A document for the percolator: term -> ascending positions.  Its proxy applies the device's phrase rule (the Phrase iterator's: some position p != 0 of
        // the first word has p + j among the positions of word j), so that the host recursion and the device answer the same question.
        using percolator_document = std::vector<std::pair<std::string, std::vector<tokenpos_t>>>;
        class percolator_positions_proxy final : public percolator_document_proxy {
              public:
                percolator_positions_proxy(const percolator_query &q, const percolator_document &d) : q(q) {
                        for (const auto &kv : d)
                                by_term[kv.first] = &kv.second;
                }
                bool match_term(const uint16_t term) override { return by_term.count(q.term_by_index(term)) != 0; }
                bool match_phrase(const uint16_t *terms, const uint16_t n) override {
                        std::vector<const std::vector<tokenpos_t> *> p(n);
                        for (uint16_t j = 0; j < n; ++j) {
                                const auto it = by_term.find(q.term_by_index(terms[j]));
                                if (it == by_term.end())
                                        return false;
                                p[j] = it->second;
                        }
                        for (const tokenpos_t at : *p[0]) {
                                bool ok = at != 0;
                                for (uint32_t j = 1; j < n && ok; ++j)
                                        ok = uint32_t(at) + j <= 0xffffu && std::binary_search(p[j]->begin(), p[j]->end(), tokenpos_t(at + j));
                                if (ok)
                                        return true;
                        }
                        return false;
                }

              private:
                const percolator_query &q;
                std::unordered_map<std::string, const std::vector<tokenpos_t> *> by_term;
        };

        // A resident set of stored queries on the device (tri_perc_create / tri_perc_match): add() queries, commit() once, match() batches of documents.
        class PercolatorSet final {
              public:
                struct match_pair {
                        uint32_t query, document;
                };
                explicit PercolatorSet(tri_dev *device) : dev(device) {}
                ~PercolatorSet() { tri_perc_destroy(h); }
                PercolatorSet(const PercolatorSet &) = delete;
                PercolatorSet &operator=(const PercolatorSet &) = delete;
                // returns the query's index in the set: what match() reports
                uint32_t add(const percolator_query &q) {
                        if (h)
                                throw invalid_argument("PercolatorSet::add after commit");
                        first.push_back({uint32_t(prog.size()), uint32_t(q.program().size())});
                        for (const uint32_t t : q.program())
                                prog.push_back((t >> 28) == TRI_OP_TERM ? TRI_TOK(TRI_OP_TERM, intern(q.term_by_index(uint16_t(t & 0x0fffffffu)))) : t);
                        return uint32_t(first.size() - 1);
                }
                void commit() {
                        if (h)
                                throw invalid_argument("PercolatorSet::commit twice");
                        check(tri_perc_create(dev, prog.data(), prog.size(), first.data(), first.size(), uint32_t(dict.size()), &h));
                }
                void set_enabled(const std::vector<uint32_t> &queries, const bool on) { check(tri_perc_set_enabled(h, queries.data(), queries.size(), on)); }
                std::vector<int32_t> status() const {
                        std::vector<int32_t> st(first.size());
                        check(tri_perc_query_status(h, st.data()));
                        return st;
                }
                // every (query, document) pair that matches; order: TRI_PERC_BY_QUERY / TRI_PERC_BY_DOCUMENT
                std::vector<match_pair> match(const std::vector<percolator_document> &documents, const int order = TRI_PERC_BY_QUERY) const {
                        if (!h)
                                throw invalid_argument("PercolatorSet::match before commit");
                        std::vector<uint64_t> doc_first{0};
                        std::vector<uint32_t> terms, freqs;
                        std::vector<tokenpos_t> positions;
                        std::vector<std::pair<uint32_t, const std::vector<tokenpos_t> *>> row;
                        for (const percolator_document &d : documents) {
                                row.clear();
                                for (const auto &kv : d) {
                                        const auto it = dict.find(kv.first);
                                        if (it != dict.end()) // (a term no stored query names: nothing can ask for it)
                                                row.emplace_back(it->second, &kv.second);
                                }
                                std::sort(row.begin(), row.end());
                                for (const auto &r : row) {
                                        terms.push_back(r.first);
                                        freqs.push_back(uint32_t(r.second->size()));
                                        positions.insert(positions.end(), r.second->begin(), r.second->end());
                                }
                                doc_first.push_back(terms.size());
                        }
                        tri_perc_docs D{};
                        D.ndocs = uint32_t(documents.size());
                        D.doc_first = doc_first.data(), D.terms = terms.data(), D.freqs = freqs.data(), D.positions = positions.data(), D.npositions = positions.size();
                        tri_perc_result *r = nullptr;
                        check(tri_perc_match(h, &D, &r));
                        struct Free {
                                tri_perc_result *r;
                                ~Free() { tri_perc_result_destroy(r); }
                        } guard{r};
                        size_t n = 0;
                        check(tri_perc_result_pairs(r, order, nullptr, nullptr, 0, &n));
                        std::vector<uint32_t> q(n + 1), d(n + 1);
                        check(tri_perc_result_pairs(r, order, q.data(), d.data(), n, &n));
                        std::vector<match_pair> out(n);
                        for (size_t i = 0; i < n; ++i)
                                out[i] = {q[i], d[i]};
                        return out;
                }

              private:
                uint32_t intern(const std::string &s) { return dict.emplace(s, uint32_t(dict.size())).first->second; }
                tri_dev *dev;
                tri_perc *h{nullptr};
                std::vector<uint32_t> prog;
                std::vector<tri_query> first;
                std::unordered_map<std::string, uint32_t> dict;
        };
} // namespace trinity_amd
