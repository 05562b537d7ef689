"""Mirror of gp/classification/GpClassifier.scala on top of libgpcore.so."""
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np

from ... import default_context
from ...core import EpClassifierState
from .ep_parameter_estimator import EpEstimationContext, EpParameterEstimator, SiteParams


@dataclass
class ClassifierInput:   # :63-65
    trainKernelMatrix: np.ndarray
    targets: np.ndarray
    initHyperParams: Any = None
    trainData: Optional[np.ndarray] = None


@dataclass
class AfterEstimationClassifierInput:   # :58-61
    targets: np.ndarray
    learnParams: Optional[Tuple[SiteParams, np.ndarray]]
    hyperParams: Any
    trainKernelMatrix: np.ndarray
    testTrainKernelMatrix: np.ndarray
    testKernelMatrix: np.ndarray


class GpClassifier:
    def __init__(self, stopCriterion):
        self.stopCriterion = stopCriterion

    def trainClassifier(self, classInput):   # :18-22 ; targets must contain values from set {-1,1}
        return EpParameterEstimator(classInput.trainKernelMatrix, classInput.targets, self.stopCriterion).estimateSiteParams()

    def classify(self, input):   # :24-47 -> probabilities of class 1
        K = np.asfortranarray(np.asarray(input.trainKernelMatrix, dtype=np.float64))
        Ks = np.asfortranarray(np.asarray(input.testTrainKernelMatrix, dtype=np.float64))
        kss = np.ascontiguousarray(np.diag(np.asarray(input.testKernelMatrix, dtype=np.float64)))
        if input.learnParams is None:
            (site, _), st = EpParameterEstimator(K, input.targets, self.stopCriterion).estimateSiteParams(keep_state=True)
        else:
            # site parameters are given: rebuild the device state (L, Sigma) from them with one refactorisation
            site, _ = input.learnParams
            st = EpClassifierState(default_context(), K, input.targets)
            st.load_site_params(site.tauSiteParams, site.niSiteParams)
        try:
            return st.predict(Ks, kss)
        finally:
            st.close()

    def classifyFromData(self, trainData, targets, hyperParams, testData, learnParams=None, max_sweeps=1000):
        """classify (:24-47) from DATA with the ARD-RBF kernel at hyperParams (sf, l_1..l_d, sn -- a vector or anything with
        toDenseVector()), as the reference's callers build their matrices: the train Gram matrix and the test-train block are built
        on the device.  learnParams = None runs EP under the stop criterion like trainClassifier."""
        X = np.asarray(trainData, dtype=np.float64)
        Xs = np.asarray(testData, dtype=np.float64)
        y = np.asarray(targets, dtype=np.int32).reshape(-1)
        theta = hyperParams.toDenseVector() if hasattr(hyperParams, "toDenseVector") else hyperParams
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        if X.ndim != 2 or Xs.ndim != 2 or X.shape[0] != y.size or Xs.shape[1] != X.shape[1] or theta.size != X.shape[1] + 2:
            raise ValueError("requirement failed: trainData n x d, targets n, testData m x d, d + 2 hyper-parameters")
        st = EpClassifierState.from_inputs(default_context(), X, y, theta)
        try:
            if learnParams is not None:
                site, _ = learnParams
                st.load_site_params(site.tauSiteParams, site.niSiteParams)
            else:
                n = y.size
                cur = SiteParams(np.zeros(n), np.zeros(n))
                old = cur
                j = 0
                while j == 0 or (j < max_sweeps and not self.stopCriterion(EpEstimationContext(oldParams=old, currentParams=cur))):
                    old = cur
                    cur = SiteParams(*st.sweep(1))
                    j += 1
            return st.predict_inputs(Xs)
        finally:
            st.close()
