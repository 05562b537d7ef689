package gp.classification

import breeze.linalg.{DenseMatrix, DenseVector}
import gp.classification.EpParameterEstimator.SiteParams
import gpcore.Native
import utils.KernelRequisites.KernelFuncHyperParams

/** Drop-in body for gp.classification.GpClassifier (gp/classification/GpClassifier.scala:11-67). */
class GpClassifier(stopCriterion: EpParameterEstimator.stopCriterionFunc) {
  import GpClassifier._
  import Native.{defaultCtx => ctx, dense, rethrowNotPd}

  /* targets must contain values from set {-1,1} */
  def trainClassifier(classInput: ClassifierInput): learnParams =
    new EpParameterEstimator(classInput.trainKernelMatrix, classInput.targets, stopCriterion).estimateSiteParams

  // :24-47 -- z, fMean, V = L \ (S^1/2 K*^T), p_i = Phi(mu*_i / sqrt(1 + var*_i)) in ONE library call; only the diagonal of
  // testKernelMatrix is read by the reference (:43-45), so only the diagonal crosses the boundary
  def classify(input: AfterEstimationClassifierInput): classifyOut = {
    val (siteParams, _) = input.learnParams.getOrElse(
      trainClassifier(ClassifierInput(trainKernelMatrix = input.trainKernelMatrix, targets = input.targets,
        initHyperParams = input.hyperParams, trainData = None)))
    val k = dense(input.trainKernelMatrix); val ks = dense(input.testTrainKernelMatrix)
    val n = k.rows; val m = ks.rows
    val ep = Native.epCreate(ctx, k.data, k.offset, n, k.majorStride, input.targets.toArray)
    try {
      rethrowNotPd { Native.epSetSiteParams(ctx, ep, n, siteParams.tauSiteParams.toArray, siteParams.niSiteParams.toArray) }
      val kssDiag = Array.tabulate(m)(i => input.testKernelMatrix(i, i))
      val prob = new Array[Double](m)
      Native.epPredict(ctx, ep, ks.data, ks.offset, m, n, ks.majorStride, kssDiag, prob)
      DenseVector(prob)
    } finally Native.epDestroy(ep)
  }

  // The same (:24-47) from DATA with the ARD-RBF kernel at hyperParams, as the reference's callers build their matrices
  // (CancerClassificationTest; MarginalLikelihoodEvaluator.scala:37): the train Gram and the test-train block are built on the
  // device and never cross the boundary.  learnParams = None runs the sweeps under stopCriterion as trainClassifier does.
  def classifyFromData(trainData: DenseMatrix[Double], targets: DenseVector[Int], hyperParams: KernelFuncHyperParams,
                       testData: DenseMatrix[Double], learnParams: Option[learnParams] = None): classifyOut = {
    require(trainData.rows == targets.length && trainData.cols == testData.cols)
    val x = dense(trainData); val xs = dense(testData)
    val n = x.rows; val m = xs.rows
    val ep = Native.epCreateRbf(ctx, x.data, x.offset, n, x.cols, x.majorStride, targets.toArray, hyperParams.toDenseVector.toArray)
    try {
      learnParams match {
        case Some((site, _)) =>
          rethrowNotPd { Native.epSetSiteParams(ctx, ep, n, site.tauSiteParams.toArray, site.niSiteParams.toArray) }
        case None =>
          var current = SiteParams(DenseVector.zeros[Double](n), DenseVector.zeros[Double](n))
          var old = current
          var j = 0
          while (j == 0 || !stopCriterion(EpParameterEstimator.EpEstimationContext(currentParams = current, oldParams = old))) {
            old = current
            val tau = new Array[Double](n); val nu = new Array[Double](n)
            rethrowNotPd { Native.epSweep(ctx, ep, 1, n, tau, nu) }
            current = SiteParams(DenseVector(tau), DenseVector(nu))
            j += 1
          }
      }
      val prob = new Array[Double](m)
      Native.epPredictRbf(ctx, ep, xs.data, xs.offset, m, xs.cols, xs.majorStride, prob)
      DenseVector(prob)
    } finally Native.epDestroy(ep)
  }
}

object GpClassifier {
  type classifyOut = DenseVector[Double]
  /* second elem from tuple is an output from cholesky decomposition */
  type learnParams = (SiteParams, DenseMatrix[Double])

  case class AfterEstimationClassifierInput(targets: DenseVector[Int], learnParams: Option[learnParams],
                                            hyperParams: KernelFuncHyperParams, trainKernelMatrix: DenseMatrix[Double],
                                            testTrainKernelMatrix: DenseMatrix[Double], testKernelMatrix: DenseMatrix[Double])
  case class ClassifierInput(trainKernelMatrix: DenseMatrix[Double], targets: DenseVector[Int],
                             initHyperParams: KernelFuncHyperParams, trainData: Option[DenseMatrix[Double]])
}
