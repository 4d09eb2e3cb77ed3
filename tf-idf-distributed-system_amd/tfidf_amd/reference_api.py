"""Host-side mirror of the reference's hot-path interface, over the GPU engine.

Java cannot be built in this image, so the reference's own host classes are
mirrored here with the same names, argument meaning and error behaviour, each
method citing the reference code it stands in for (paths relative to
TF-IDF-System-Core/src/main/java/).  INTEGRATION.md shows the JNI binding a
maintainer adds to the Java classes themselves.

  Worker  <- me/zookeeper/leader_election/worker/Worker.java
  Leader  <- me/zookeeper/leader_election/leader/Leader.java
  DocumentScoreInfo JSON <- Document_and_Data/DocumentScoreInfo.java:11-31,
                            Document_and_Data/Document.java:6-53
"""
import os
import re

from . import _lib as L
from .engine import ShardIndex, analyze, leader_merge, query_positive_terms


def extract_text(data: bytes) -> bytes:
    """Stand-in for the reference's Tika fallback (AutoDetectParser +
    BodyContentHandler, Worker.java:201-211) on a file that is not valid
    UTF-8: plain text in a single-byte Western encoding is decoded as
    windows-1252 (bytes it leaves undefined as Latin-1) and re-encoded as
    UTF-8.  Tika's own charset detection and its parsers for binary formats
    (PDF, Office) are not rebuilt: parity unpinned."""
    out = []
    for b in data:
        try:
            out.append(bytes([b]).decode("cp1252"))
        except UnicodeDecodeError:
            out.append(chr(b))
    return "".join(out).encode("utf-8")


def document_score_info(name: str, score: float):
    """Jackson form of DocumentScoreInfo: {"document": {"name": ...}, "score": double}."""
    return {"document": {"name": name}, "score": float(score)}


_OCCUR_PREFIX = {"+": L.OCCUR_MUST, "-": L.OCCUR_MUST_NOT, "#": L.OCCUR_FILTER}


def _syntax(msg):
    return L.QuerySyntaxError(L.E_QUERY_SYNTAX, msg)


def _parse_clause(text, i, tree):
    """The clause that starts at text[i], after its occur prefix -> (clause, index after it).  ``tree``: the
    grammar of parse_query_tree, where an unescaped ``)`` ends a token and may follow a closing quote or slash."""
    from . import engine as E
    n = len(text)

    def ends(j):
        return j >= n or text[j].isspace() or (tree and text[j] == ")")

    if text[i] == '"':
        j = text.find('"', i + 1)
        if j < 0:
            raise _syntax("unclosed quote at %d" % i)
        body, i = text[i + 1:j], j + 1
        m = re.match(r"~(\d+)", text[i:])
        slop = 0
        if m:
            slop, i = int(m.group(1)), i + m.end()
        if not ends(i):
            raise _syntax("text after the closing quote at %d" % i)
        return E.phrase(body.encode(), min(slop, 0x7FFFFFFF)), i
    if text[i] == "/":
        j, body = i + 1, []
        while j < n and text[j] != "/":
            if text[j] == "\\" and j + 1 < n and text[j + 1] == "/":
                body.append("/")
                j += 2
                continue
            if text[j] == "\\" and j + 1 < n:          # any other escape stays the pattern's own
                body.append(text[j:j + 2])
                j += 2
                continue
            body.append(text[j])
            j += 1
        if j >= n:
            raise _syntax("unclosed slash at %d" % i)
        i = j + 1
        if not ends(i):
            raise _syntax("text after the closing slash at %d" % i)
        return E.regex("".join(body).encode()), i
    j = i
    while not ends(j):
        j += 2 if tree and text[j] == "\\" and j + 1 < n and not text[j + 1].isspace() else 1
    tok, i = text[i:j], j
    m = re.match(r"^(.+)~(\d*)$", tok, re.S)
    if m:
        edits = int(m.group(2)) if m.group(2) else 2
        if edits > 2:
            raise _syntax("fuzzy edits %d above 2 in '%s'" % (edits, tok))
        return E.fuzzy(m.group(1).lower().encode(), edits), i
    if re.search(r"(?<!\\)(?:\\\\)*[*?]", tok):
        return E.wildcard(tok.encode()), i
    return E.text(tok.encode()), i


def parse_compound_query(text: str):
    """Worker.search_query's grammar: one query string -> the clause list of
    ShardIndex.search_compound, on the host.  Clauses are separated by
    whitespace.  A prefix gives the occur: ``+`` MUST, ``-`` MUST_NOT, ``#``
    FILTER, none SHOULD.  ``"..."`` with an optional ``~N`` is a phrase with slop
    N; ``/.../`` is a regular expression (``\\/`` is a slash in it); ``word~`` or
    ``word~N`` is a fuzzy term with N edits (0..2, default 2), lower-cased; a
    token with an unescaped ``*`` or ``?`` is a wildcard pattern; anything else
    is a one-token text clause, handed on as search_index hands its query.  An
    unclosed quote or slash, a prefix without a clause, text glued to a closing
    quote or slash, or an edit count above 2 raises QuerySyntaxError."""
    out, i, n = [], 0, len(text)
    while i < n:
        if text[i].isspace():
            i += 1
            continue
        occur = L.OCCUR_SHOULD
        if text[i] in _OCCUR_PREFIX:
            occur = _OCCUR_PREFIX[text[i]]
            i += 1
            if i >= n or text[i].isspace():
                raise _syntax("a '%s' without a clause at %d" % (text[i - 1], i - 1))
        clause, i = _parse_clause(text, i, False)
        out.append((occur,) + clause)
    return out


MAX_GROUP_DEPTH = 3          # kCqnMaxDepth - 1: the root is depth 0, a group at depth 4 is invalid


def parse_query_tree(text: str):
    """Worker.search_expr's grammar: one query string -> the group(...) of
    ShardIndex.search_nested.  It is parse_compound_query's grammar plus
    groups: outside quotes and slashes, an unescaped ``(`` at the start of a
    clause, after the optional occur prefix, opens a group; an unescaped ``)``
    ends the current token and closes the group; ``~N`` right after the ``)``
    sets the group's min_should_match.  After ``)`` or ``)~N`` only whitespace,
    another ``)`` or the end may follow.  ``\\(`` and ``\\)`` stay in the token as
    written; ``()`` is an empty group.  Unbalanced parentheses, groups nested
    deeper than 3 below the root, a prefix before ``)`` and text glued after
    ``)`` raise QuerySyntaxError, beside what parse_compound_query raises.  A
    string without groups parses to group(parse_compound_query(text))."""
    from . import engine as E
    n = len(text)

    def children_from(i, depth):
        """-> (children, index after them, whether a ')' closed them)."""
        out = []
        while i < n:
            if text[i].isspace():
                i += 1
                continue
            if text[i] == ")":
                if depth == 0:
                    raise _syntax("a ')' without its '(' at %d" % i)
                return out, i + 1, True
            occur = L.OCCUR_SHOULD
            if text[i] in _OCCUR_PREFIX:
                occur = _OCCUR_PREFIX[text[i]]
                i += 1
                if i >= n or text[i].isspace() or text[i] == ")":
                    raise _syntax("a '%s' without a clause at %d" % (text[i - 1], i - 1))
            if text[i] != "(":
                clause, i = _parse_clause(text, i, True)
                out.append((occur,) + clause)
                continue
            if depth >= MAX_GROUP_DEPTH:
                raise _syntax("groups nested deeper than %d at %d" % (MAX_GROUP_DEPTH, i))
            sub, j, closed = children_from(i + 1, depth + 1)
            if not closed:
                raise _syntax("unclosed '(' at %d" % i)
            i, m = j, re.match(r"~(\d+)", text[j:])
            msm = 0
            if m:
                msm, i = min(int(m.group(1)), 0xFFFFFFFF), i + m.end()
            if i < n and not text[i].isspace() and text[i] != ")":
                raise _syntax("text after the closing ')' at %d" % i)
            out.append((occur,) + E.group(sub, msm))
        return out, i, False

    return E.group(children_from(0, 0)[0])


class Worker:
    """Worker.java:42-242 — one shard: builds its index at init, answers
    /worker/process with every hit of its shard-local BM25 ranking."""

    def __init__(self, documents_path=None, index_path=None, device=0, vocab_capacity_log2=18,
                 compact_threshold_pct=0):
        # @Value("${mydocument.path}") / @Value("${lucene.index.path}") (Worker.java:48-52)
        self.DOCUMENTS_PATH = documents_path
        self.INDEX_PATH = index_path
        self.index = ShardIndex(device=device, vocab_capacity_log2=vocab_capacity_log2)
        # uploads overwrite files by name (Worker.java:133-138): with a threshold
        # the commit reclaims the replaced versions, as Lucene's merges do
        if compact_threshold_pct:
            self.index.set_compact_threshold(compact_threshold_pct)
        self._committed = False

    INDEX_FILE = "tfidf.idx"

    def _index_file(self):
        return os.path.join(self.INDEX_PATH, self.INDEX_FILE) if self.INDEX_PATH else None

    # Worker.java:57-94 @PostConstruct init: open the index directory
    # (IndexWriterConfig default OpenMode CREATE_OR_APPEND: a saved index is
    # reopened), walk the documents directory skipping the index directory,
    # addDocToIndex per regular file (replacing by relative path), commit.
    def init(self):
        idx_file = self._index_file()
        if idx_file and os.path.isfile(idx_file):
            self.index.load(idx_file)
        docs_path = os.path.normpath(self.DOCUMENTS_PATH)
        if not os.path.isdir(docs_path):
            if idx_file and os.path.isfile(idx_file):
                self.commit()
            return
        idx_path = os.path.normpath(self.INDEX_PATH) if self.INDEX_PATH else None
        paths = []
        # Files.walk order is file-system dependent; sorted depth-first here so
        # document ids (tie-break order) are reproducible.
        for root, dirs, files in os.walk(docs_path):
            dirs.sort()
            if idx_path and os.path.normpath(root).startswith(idx_path):
                continue
            dirs[:] = [d for d in dirs if not (idx_path and os.path.join(root, d).startswith(idx_path))]
            for f in sorted(files):
                paths.append(os.path.join(root, f))
        keys, texts = [], []
        for p in paths:
            try:
                k, t = self._read(p)
            except OSError:
                continue                      # Worker.java:83-85: log and skip
            keys.append(k)
            texts.append(t)
        self.index.add_documents(texts, keys)
        self.commit()

    def _read(self, path):
        base = os.path.normpath(self.DOCUMENTS_PATH)
        absp = os.path.normpath(path)
        # Worker.java:191-195: RELATIVE path is the document key
        rel = os.path.relpath(absp, base) if absp.startswith(base + os.sep) else os.path.basename(absp)
        with open(absp, "rb") as f:
            data = f.read()
        try:
            data.decode("utf-8")              # Files.readString: strict UTF-8
        except UnicodeDecodeError:
            data = extract_text(data)         # MalformedInputException -> Tika (Worker.java:199-211)
        return rel.encode(), data

    # Worker.java:190-220 addDocToIndex (updateDocument by Term("path", rel))
    def add_doc_to_index(self, path):
        k, t = self._read(path)
        self.index.add_documents([t], [k])

    # Worker.java:88,138 indexWriter.commit(): the index becomes durable
    def commit(self):
        self.index.commit()
        self._committed = True
        idx_file = self._index_file()
        if idx_file:
            os.makedirs(self.INDEX_PATH, exist_ok=True)
            self.index.save(idx_file)

    # Worker.java:125-146 upload: copy the file, then add + commit under the writer lock
    def upload(self, filename, data: bytes):
        if not data:
            return 400, "Empty file"
        try:
            dest = os.path.normpath(os.path.join(self.DOCUMENTS_PATH, filename))
            with open(dest, "wb") as f:
                f.write(data)
            self.add_doc_to_index(dest)
            self.commit()
            return 200, "Uploaded"
        except Exception as e:                # Worker.java:142-145
            return 500, "Upload failed: %s" % e

    # Worker.java:147-172 /worker/index-size (bytes held by the index)
    def get_index_size(self):
        return int(self.index.stats()["device_bytes"]) if self._committed else 0

    # Worker.java:222-241 searchIndex: every hit, score desc / doc asc
    def search_index(self, query: str):
        # one reader per request: hits and their stored paths from the same commit (:223, :234-238)
        with self.index.reader() as rd:
            hits = rd.search(query.encode(), 0)
            return [document_score_info(rd.doc_key(d).decode(), s) for d, s in hits]

    # No reference counterpart (QueryParser.escape neutralises the quotes,
    # Worker.java:225-227): the documents that hold the analysed words of
    # ``query`` next to each other in order, every hit, in the order and shape
    # of search_index; DocumentScoreInfo JSON extended with "freq" (the
    # phrase's occurrences in the document).
    def search_phrase(self, query: str):
        with self.index.reader() as rd:
            out = []
            for d, s, f in rd.search_phrase(query.encode()):
                info = document_score_info(rd.doc_key(d).decode(), s)
                info["freq"] = f
                out.append(info)
            return out

    # No reference counterpart: search_phrase with Lucene's slop (the words of
    # ``query`` within ``slop`` position moves of the phrase, in any order once
    # the slop allows it); "freq" is SloppyPhraseMatcher's float frequency.
    # With slop > 0 a query that repeats a word or has more than 64 words is a
    # ValueError.
    def search_near(self, query: str, slop: int):
        with self.index.reader() as rd:
            try:
                hits = rd.search_phrase_slop(query.encode(), slop)
            except L.TfidfError as e:
                if e.code == L.E_UNSUPPORTED_QUERY:
                    raise ValueError(str(e)) from None
                raise
            out = []
            for d, s, f in hits:
                info = document_score_info(rd.doc_key(d).decode(), s)
                info["freq"] = f
                out.append(info)
            return out

    # No reference counterpart (QueryParser.escape neutralises every operator):
    # one query string of mixed clauses (parse_compound_query), combined by
    # Lucene's flat BooleanQuery rule on the device; the first ``k`` hits (0 =
    # all) in the order and shape of search_index.  A string that does not
    # parse raises QuerySyntaxError, as search_index's query does.
    def search_query(self, text: str, k=10):
        clauses = parse_compound_query(text)
        with self.index.reader() as rd:
            hits = rd.search_compound(clauses)
            return [document_score_info(rd.doc_key(d).decode(), s) for d, s in (hits[:k] if k else hits)]

    # search_query with clause groups: ``(...)`` groups clauses, ``)~N`` asks for
    # N of the group's SHOULD clauses (parse_query_tree); ``min_should_match``
    # is the whole string's.  The tree is evaluated on the device as written.
    def search_expr(self, text: str, k=10, min_should_match=0):
        from . import engine as E
        query = E.group(parse_query_tree(text)[1], min_should_match)
        with self.index.reader() as rd:
            hits = rd.search_nested(query)
            return [document_score_info(rd.doc_key(d).decode(), s) for d, s in (hits[:k] if k else hits)]

    # No reference counterpart ("contents" has no term vectors, so Lucene's
    # MoreLikeThis.like(docNum) would find no terms there): the ``k``
    # documents most like the document whose key is ``name``, without that
    # document, in the shape of search_index; [] for a name the index lacks.
    # Key and hits are resolved on one reader.
    def search_similar(self, name: str, k=10):
        with self.index.reader() as rd:
            blob, offs = rd.doc_keys()
            raw, o, key = blob.tobytes(), offs.tolist(), name.encode()
            doc = next((d for d in range(rd.num_docs) if raw[o[d]:o[d + 1]] == key), None)
            if doc is None:
                return []
            return [document_score_info(rd.doc_key(d).decode(), s) for d, s in rd.more_like_this(doc, k)]

    # No reference counterpart ("contents" is stored with Store.NO,
    # Worker.java:216): the top-k hits with the passage that shows why each
    # matched, search and snippets on one reader.  DocumentScoreInfo JSON
    # extended with "snippet" (str) and "matches" ([[start, len], ...] in
    # snippet bytes).
    def search_snippets(self, query: str, k=10, max_bytes=160):
        q = query.encode()
        with self.index.reader() as rd:
            hits = rd.search(q, k)
            snips = rd.snippets(q, [d for d, _ in hits], max_bytes)
            out = []
            for (d, s), (_, text, ms) in zip(hits, snips):
                info = document_score_info(rd.doc_key(d).decode(), s)
                info["snippet"] = text.decode("utf-8", errors="replace")
                info["matches"] = [[st, ln] for st, ln, _ in ms]
                out.append(info)
            return out

    # search_snippets for the requests of concurrent threads in one pass: one
    # reader, one batched all-hits search, the first k hits of each query, one
    # batched snippets call for all of them.  A request whose query fails
    # yields [] (as in process_documents_batch).
    def search_snippets_batch(self, queries, k=10, max_bytes=160):
        out = [[] for _ in queries]
        enc, at = [], []
        for i, q in enumerate(queries):
            try:
                enc.append(q.encode())
                at.append(i)
            except Exception:
                pass
        with self.index.reader() as rd:
            top = [hits[:k] if k else hits for hits in rd.search_batch_all(enc)]
            snips = rd.snippets_batch(enc, [[d for d, _ in hits] for hits in top], max_bytes)
            names = {}
            for i, hits, sn in zip(at, top, snips):
                for (d, s), (_, text, ms) in zip(hits, sn):
                    if d not in names:
                        names[d] = rd.doc_key(d).decode()
                    info = document_score_info(names[d], s)
                    info["snippet"] = text.decode("utf-8", errors="replace")
                    info["matches"] = [[st, ln] for st, ln, _ in ms]
                    out[i].append(info)
        return out

    # No reference counterpart (QueryParser.escape neutralises '~'): a query
    # whose terms are misspelt is answered with the nearest spelling the index
    # holds.  Every positive term of the query is looked up in one batched
    # fuzzy call; a term that is not in the vocabulary itself is replaced by
    # its first candidate (distance, then df, then bytes), if it has one.
    # -> (corrected query or None, hits of the corrected-or-original query)
    def search_did_you_mean(self, query: str, max_edits=2):
        q = query.encode()
        with self.index.reader() as rd:
            terms = query_positive_terms(q)
            corrected = query
            for t, (cands, _) in zip(terms, rd.fuzzy_terms_batch(terms, max_edits, 0, 1)):
                if cands and cands[0][2] != 0:
                    # the misspelt word where the query spells it (any case): operators and boosts stay
                    best = cands[0][0].decode()
                    corrected = re.sub(r"(?<!\w)%s(?!\w)" % re.escape(t.decode()), lambda m: best, corrected,
                                       flags=re.IGNORECASE)
            changed = corrected != query
            hits = rd.search(corrected.encode() if changed else q, 0)
            out = [document_score_info(rd.doc_key(d).decode(), s) for d, s in hits]
        return (corrected if changed else None), out

    # No reference counterpart (QueryParser.escape neutralises '~'): Lucene's
    # FuzzyQuery on the one word ``word`` analyses to: the documents holding
    # any of the max_expansions closest spellings within max_edits, a closer
    # spelling weighing more and all weighted with the most frequent one's idf;
    # every hit in the order and shape of search_index.  Text that analyses to
    # no word or to several is a ValueError.
    def search_fuzzy(self, word: str, max_edits=2, prefix_len=0, max_expansions=50):
        tokens = analyze(word.encode())
        if len(tokens) != 1:
            raise ValueError("fuzzy search takes exactly one word, got %d" % len(tokens))
        with self.index.reader() as rd:
            hits = rd.search_fuzzy(tokens[0], max_edits, prefix_len, max_expansions)
            return [document_score_info(rd.doc_key(d).decode(), s) for d, s in hits]

    # No reference counterpart (QueryParser.escape neutralises '*' and '?'):
    # the documents holding a term that starts with ``text`` (lower-cased, not
    # tokenised; its own '*', '?' and '\' are literals), every hit with the
    # constant score 1.0 in doc id order, in the shape of search_index.
    def search_prefix(self, text: str):
        pattern = re.sub(r"([*?\\])", r"\\\1", text).encode() + b"*"
        with self.index.reader() as rd:
            docs, _ = rd.search_wildcard(pattern)
            return [document_score_info(rd.doc_key(d).decode(), 1.0) for d in docs]

    # No reference counterpart: the documents holding a term of the regular
    # expression's language (Lucene's RegExp syntax; the pattern is not
    # lower-cased), every hit with the constant score 1.0 in doc id order, in
    # the shape of search_prefix.  A pattern in error raises TfidfError.
    def search_regex(self, pattern: str):
        with self.index.reader() as rd:
            docs, _ = rd.search_regex(pattern.encode())
            return [document_score_info(rd.doc_key(d).decode(), 1.0) for d in docs]

    # The type-ahead call: the ``n`` most frequent vocabulary terms that start
    # with ``prefix`` (df descending, then bytes) -> [(term, df)]
    def suggest_terms(self, prefix: str, n=10):
        pattern = re.sub(r"([*?\\])", r"\\\1", prefix).encode() + b"*"
        with self.index.reader() as rd:
            terms, _ = rd.wildcard_terms(pattern, n)
            return [(t.decode("utf-8", errors="replace"), df) for t, df in terms]

    # Worker.java:175-186 /worker/process: any exception -> empty list
    def process_documents(self, search_query: str):
        try:
            return self.search_index(search_query)
        except Exception:
            return []

    # /worker/process for the requests of concurrent threads (Worker.java:175-186,
    # cfg 4) in one pass: process_documents(q) for each query, every hit of all
    # of them from one batched all-hits search on one reader
    def process_documents_batch(self, search_queries):
        out = [[] for _ in search_queries]
        enc, at = [], []
        for i, q in enumerate(search_queries):
            try:
                enc.append(q.encode())
                at.append(i)
            except Exception:
                pass                          # that request's exception -> its empty list
        try:
            with self.index.reader() as rd:
                names = {}
                for i, hits in zip(at, rd.search_batch_all(enc)):
                    for d, _ in hits:
                        if d not in names:
                            names[d] = rd.doc_key(d).decode()
                    out[i] = [document_score_info(names[d], s) for d, s in hits]
        except Exception:
            return [[] for _ in search_queries]
        return out

    def close(self):
        self.index.close()


class Leader:
    """Leader.java:39-92 /leader/start: fan the query out to every worker
    (sequentially; failed workers are skipped), sum scores per document name
    in double, return the map ordered by name."""

    def __init__(self, workers, node=None):
        self.workers = workers                # ServiceRegistry.getAllServiceAddresses()
        self.node = node                      # a SHARD-mode distributed.Node holding the workers' shards

    # /leader/start for the requests of concurrent threads in one pass:
    # start(q) for each query.  Over a node (SHARD statistics: one shard per
    # worker) the fan-out and the merge of the whole batch are one
    # Node.search_names_batch; a query that fails on the workers (ParseException)
    # merges nothing, as every worker answers [] for it (Worker.java:182-185).
    def start_batch(self, search_queries):
        if self.node is None:
            return [self.start(q) for q in search_queries]
        out = [{} for _ in search_queries]
        enc, at = [], []
        for i, q in enumerate(search_queries):
            try:
                enc.append(q.encode())
                at.append(i)
            except Exception:
                pass                          # that request's exception on every worker -> {}
        for i, merged in zip(at, self.node.search_names_batch(enc)):
            out[i] = {name.decode(): score for name, score in merged}
        return out

    def start(self, search_query: str):
        if not self.workers:
            return {}                         # Leader.java:45-48
        responses = []
        for w in self.workers:
            try:
                resp = w.process_documents(search_query)
            except Exception:
                continue                      # Leader.java:67-69
            if resp is None:
                continue
            responses.append([(r["document"]["name"].encode(), r["score"]) for r in resp])
        merged = leader_merge(responses)      # Leader.java:73-88
        return {name.decode(): score for name, score in merged}


__all__ = ["Worker", "Leader", "document_score_info", "L"]
