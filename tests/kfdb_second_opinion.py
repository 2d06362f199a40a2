"""A second opinion on the keyframe database, in plain Python, written from the text of the reference's
src/KeyFrameDatabase.cc:41-310 and Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68: one list of keyframes per word, the per-keyframe
bookkeeping fields under the reference's names, `score` as a sequential loop over Python floats (doubles) and np.float32
wherever the reference holds a `float`.  It shares no code with pointslot_amd.  mRelocScore is 0.0 at construction: the stated
modelling choice where the reference leaves the member uninitialised (include/pointslot_hip.h, the keyframe database section).

Besides the candidates every query returns a trace: the sharing list with words and scores as ps_kfdb_query reports them, and
tallies of the branches taken in the covisibility stage, which the tests use to show that the cases are not vacuous."""
import numpy as np

F32 = np.float32


class KeyFrame:
    def __init__(self, mnId, bow_id=(), bow_val=()):
        self.mnId = int(mnId)
        self.mBowVec = [(int(w), float(v)) for w, v in zip(bow_id, bow_val)]     # std::map order: ascending word id
        self.mnLoopQuery = -1
        self.mnLoopWords = 0
        self.mLoopScore = F32(0.0)
        self.mnRelocQuery = -1
        self.mnRelocWords = 0
        self.mRelocScore = F32(0.0)
        self.neigh = []          # GetBestCovisibilityKeyFrames(10): KeyFrame objects, stored in the database or not
        self.connected = set()   # GetConnectedKeyFrames(): KeyFrame objects (a query keyframe's)

    def GetBestCovisibilityKeyFrames(self, n):
        return self.neigh[:n]


def score(v1, v2):
    """L1Scoring::score on two ascending (word, value) lists"""
    i, j = 0, 0
    s = 0.0
    while i < len(v1) and j < len(v2):
        vi, wi = v1[i][1], v2[j][1]
        if v1[i][0] == v2[j][0]:
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif v1[i][0] < v2[j][0]:
            while i < len(v1) and v1[i][0] < v2[j][0]:      # v1.lower_bound(v2_it->first)
                i += 1
        else:
            while j < len(v2) and v2[j][0] < v1[i][0]:
                j += 1
    s = -s / 2.0
    return s


class KeyFrameDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.mvInvertedFile = [[] for _ in range(nwords)]

    def add(self, pKF):
        for w, _ in pKF.mBowVec:
            self.mvInvertedFile[w].append(pKF)

    def erase(self, pKF):
        for w, _ in pKF.mBowVec:
            lKFs = self.mvInvertedFile[w]
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = [[] for _ in range(self.nwords)]

    def DetectLoopCandidates(self, pKF, minScore):
        minScore = F32(minScore)
        trace = dict(mode=1, share=[], words=[], score=[], min_common_words=0, best_is_neighbour=0, duplicates=0, rejected=0, stale_reads=0,
                     excluded_words=0)
        spConnectedKeyFrames = pKF.connected
        lKFsSharingWords = []
        for w, _ in pKF.mBowVec:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != pKF.mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF.mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        # (a connected keyframe's counter is reset at every word, so it ends at 1; its true count, for the tests only)
        mine = set(w for w, _ in pKF.mBowVec)
        for c in spConnectedKeyFrames:
            trace["excluded_words"] = max(trace["excluded_words"], sum(1 for w, _ in c.mBowVec if w in mine and c in self.mvInvertedFile[w]))
        trace["share"] = [k.mnId for k in lKFsSharingWords]
        trace["words"] = [k.mnLoopWords for k in lKFsSharingWords]
        trace["score"] = [F32(0.0)] * len(lKFsSharingWords)
        if not lKFsSharingWords:
            return [], trace
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        trace["min_common_words"] = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(score(pKF.mBowVec, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        trace["score"] = [k.mLoopScore if k.mnLoopWords > minCommonWords else F32(0.0) for k in lKFsSharingWords]
        if not lScoreAndMatch:
            return [], trace
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnLoopQuery == pKF.mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            trace["best_is_neighbour"] += pBestKF is not pKFi
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore, trace), trace

    def DetectRelocalizationCandidates(self, F):
        trace = dict(mode=0, share=[], words=[], score=[], min_common_words=0, best_is_neighbour=0, duplicates=0, rejected=0, stale_reads=0,
                     excluded_words=0)
        lKFsSharingWords = []
        for w, _ in F.mBowVec:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        trace["share"] = [k.mnId for k in lKFsSharingWords]
        trace["words"] = [k.mnRelocWords for k in lKFsSharingWords]
        trace["score"] = [k.mRelocScore for k in lKFsSharingWords]
        if not lKFsSharingWords:
            return [], trace
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        trace["min_common_words"] = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(score(F.mBowVec, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        trace["score"] = [k.mRelocScore for k in lKFsSharingWords]
        if not lScoreAndMatch:
            return [], trace
        lAccScoreAndMatch = []
        bestAccScore = F32(0.0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                summed = F32(accScore + pKF2.mRelocScore)
                if not pKF2.mnRelocWords > minCommonWords and pKF2.mRelocScore != 0 and summed != accScore:
                    trace["stale_reads"] += 1        # not scored by this query: what an earlier query left
                accScore = summed
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            trace["best_is_neighbour"] += pBestKF is not pKFi
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore, trace), trace

    @staticmethod
    def _retain(lAccScoreAndMatch, bestAccScore, trace):
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        out = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    out.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
                else:
                    trace["duplicates"] += 1
            else:
                trace["rejected"] += 1
        return out
