"""Sequential reference: a literal, loop-for-loop Python/numpy restatement of the extractor and of the
matchers the timed paths run, written from the reference text (src/ORBextractor.cc, src/ORBmatcher.cc,
src/Frame.cc), and of everything guided by the DBoW2 vocabulary (bow.py: loadFromTextFile and transform of
Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h with BowVector.cpp and FORB.cpp, both SearchByBoW forms,
SearchForTriangulation with CheckDistEpipolarLine).  TEST INFRASTRUCTURE ONLY.

It is independent of the C oracle on purpose: it loads no shared library and imports neither the oracle
nor the product package, so a misreading shared by those two shows up as a disagreement with this one.
Where the reference is not deterministic, or leans on OpenCV, it adopts the choices of DESIGN.md section 3
and names them where they are made.
"""
